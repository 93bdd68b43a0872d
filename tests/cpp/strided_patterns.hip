// Strided / blocked put / get through the C++ names (include/ishmem.h, include/ishmemx.h,
// include/ishmemx_device.h) in the shape of the reference's test/unit/ibput.cpp, ibget.cpp and
// int_iput_device.cpp.  Every PE puts to the next PE (me + 1) % npes, or gets from it.
//   Kinds: float, double, uint8, uint16, uint32, uint64 and the sized forms 8 .. 128.
//   Calls: the ibput tester's pair of calls for nelems = 1, 2, 3, 16, 1024 (the second call of
//   nelems = 3 has a zero stride and is left out), int_iput_device's shape (dst 3, sst 2, 5 elements)
//   and a few larger strided and blocked shapes; calls with bsize 1 marked `i` go through the
//   iput / iget names, all others through ibput / ibget.
//   Modes: host blocking, on-stream, work_group by a 256-thread block, by a 64-lane tile, single
//   threads (one call per thread, each with its own arguments), and a multi-workgroup kernel in which
//   each workgroup moves its own range of blocks.
// Every source slot holds the little-endian int64 words (slot << 48) + ((0x80 + f) << 40) +
// ((0x80 + t) << 32) + k (ishmem_tester.h:1118-1149).  The dest arena is prefilled with 0xA5; one mode
// moves all calls between two barriers and the WHOLE arena is compared on the host, so the gaps
// between strided elements and the guards must be unchanged.
// Launch: ISHMEM_PE=<pe> ISHMEM_NPES=<n> ISHMEM_DEVICE=0 ISHMEM_BOOTSTRAP_KEY=<k> ./strided_patterns
#include <hip/hip_cooperative_groups.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ishmem.h"
#include "ishmemx.h"

namespace cg = cooperative_groups;

static int errors = 0;
static long cases = 0;

constexpr size_t kGuard = 64, kSlotElems = 8192, kSlices = 8;
enum Mode { kHost = 0, kOnStream = 1, kBlock = 2, kWave = 3, kThread = 4, kMultiWg = 5, kModes = 6 };
static const char *const kModeName[kModes] = {"host", "on_stream", "work_group", "wave_tile", "thread", "multi_wg"};

struct Call {
    int slot;            // both arenas' slot
    long doe, soe;       // element offsets of dest / source in the slot
    long dst, sst;       // element strides
    size_t bsize, nblocks;
    int i;               // 1: bsize == 1 through the iput / iget names
};
// Slots 0-4: the tester's pairs for nelems 1, 2, 3, 16, 1024; 5: int_iput_device; 6-10: larger shapes.
__host__ __device__ inline int ncalls() { return 14; }
__host__ __device__ inline Call call_of(int c)
{
    switch (c) {
        case 0: return Call{0, 0, 0, 1, 1, 1, 1, 0};
        case 1: return Call{1, 0, 0, 1, 1, 1, 2, 0};
        case 2: return Call{2, 0, 0, 1, 1, 1, 2, 0};
        case 3: return Call{3, 0, 0, 8, 1, 1, 2, 0};
        case 4: return Call{3, 1, 2, 8, 7, 7, 2, 0};
        case 5: return Call{4, 0, 0, 512, 1, 1, 2, 0};
        case 6: return Call{4, 1, 2, 512, 511, 511, 2, 0};
        case 7: return Call{5, 0, 0, 3, 2, 1, 5, 1};
        case 8: return Call{6, 0, 0, 7, 1, 1, 1025, 1};
        case 9: return Call{7, 0, 0, 2, 3, 1, 2049, 1};
        case 10: return Call{8, 0, 0, 34, 69, 33, 65, 0};
        case 11: return Call{9, 0, 0, 17, 35, 16, 3, 0};
        case 12: return Call{10, 0, 0, 8, 4, 4, 777, 0};
        default: return Call{10, 6500, 4000, 5, 5, 5, 100, 0};  // both strides == bsize: contiguous
    }
}
constexpr int kSlots = 11;
static size_t slot_bytes(size_t esz) { return kSlotElems * esz + 2 * kGuard; }
static size_t arena_bytes(size_t esz) { return kSlots * slot_bytes(esz); }

// ---- the names under test, one struct per kind ------------------------------------------------
#define KIND_BODY(ESZ, LABEL, IPUT, IGET, IBPUT, IBGET, XIPUT, XIGET, XIBPUT, XIBGET, WIPUT, WIGET, WIBPUT, WIBGET) \
    static constexpr size_t esz = ESZ;                                                                          \
    static const char *name() { return LABEL; }                                                                 \
    static void host(bool put, void *d, const void *s, const Call &c, int pe)                                   \
    {                                                                                                           \
        if (c.i) put ? IPUT((ET *) d, (const ET *) s, c.dst, c.sst, c.nblocks, pe)                              \
                     : IGET((ET *) d, (const ET *) s, c.dst, c.sst, c.nblocks, pe);                             \
        else put ? IBPUT((ET *) d, (const ET *) s, c.dst, c.sst, c.bsize, c.nblocks, pe)                        \
                 : IBGET((ET *) d, (const ET *) s, c.dst, c.sst, c.bsize, c.nblocks, pe);                       \
    }                                                                                                           \
    static int on_stream(bool put, void *d, const void *s, const Call &c, int pe, hipStream_t st)               \
    {                                                                                                           \
        if (c.i) return put ? XIPUT((ET *) d, (const ET *) s, c.dst, c.sst, c.nblocks, pe, st)                  \
                            : XIGET((ET *) d, (const ET *) s, c.dst, c.sst, c.nblocks, pe, st);                 \
        return put ? XIBPUT((ET *) d, (const ET *) s, c.dst, c.sst, c.bsize, c.nblocks, pe, st)                 \
                   : XIBGET((ET *) d, (const ET *) s, c.dst, c.sst, c.bsize, c.nblocks, pe, st);                \
    }                                                                                                           \
    template <bool PUT>                                                                                         \
    __device__ static void thread(void *d, const void *s, const Call &c, int pe)                                \
    {                                                                                                           \
        if (c.i) {                                                                                              \
            if constexpr (PUT) IPUT((ET *) d, (const ET *) s, c.dst, c.sst, c.nblocks, pe);                     \
            else IGET((ET *) d, (const ET *) s, c.dst, c.sst, c.nblocks, pe);                                   \
        } else {                                                                                                \
            if constexpr (PUT) IBPUT((ET *) d, (const ET *) s, c.dst, c.sst, c.bsize, c.nblocks, pe);           \
            else IBGET((ET *) d, (const ET *) s, c.dst, c.sst, c.bsize, c.nblocks, pe);                         \
        }                                                                                                       \
    }                                                                                                           \
    template <bool PUT, typename G>                                                                             \
    __device__ static void group(void *d, const void *s, const Call &c, size_t nblocks, int pe, const G &g)     \
    {                                                                                                           \
        if (c.i) {                                                                                              \
            if constexpr (PUT) WIPUT((ET *) d, (const ET *) s, c.dst, c.sst, nblocks, pe, g);                   \
            else WIGET((ET *) d, (const ET *) s, c.dst, c.sst, nblocks, pe, g);                                 \
        } else {                                                                                                \
            if constexpr (PUT) WIBPUT((ET *) d, (const ET *) s, c.dst, c.sst, c.bsize, nblocks, pe, g);         \
            else WIBGET((ET *) d, (const ET *) s, c.dst, c.sst, c.bsize, nblocks, pe, g);                       \
        }                                                                                                       \
    }
#define KIND_TYPED(TN, TYPE)                                                                                    \
    struct K_##TN {                                                                                             \
        using ET = TYPE;                                                                                        \
        KIND_BODY(sizeof(TYPE), #TN, ishmem_##TN##_iput, ishmem_##TN##_iget, ishmemx_##TN##_ibput,              \
                  ishmemx_##TN##_ibget, ishmemx_##TN##_iput_on_stream, ishmemx_##TN##_iget_on_stream,           \
                  ishmemx_##TN##_ibput_on_stream, ishmemx_##TN##_ibget_on_stream, ishmemx_##TN##_iput_work_group, \
                  ishmemx_##TN##_iget_work_group, ishmemx_##TN##_ibput_work_group, ishmemx_##TN##_ibget_work_group) \
    };
#define KIND_SIZED(BITS)                                                                                        \
    struct K_##BITS {                                                                                           \
        using ET = void;                                                                                        \
        KIND_BODY(BITS / 8, #BITS, ishmem_iput##BITS, ishmem_iget##BITS, ishmemx_ibput##BITS, ishmemx_ibget##BITS, \
                  ishmemx_iput##BITS##_on_stream, ishmemx_iget##BITS##_on_stream, ishmemx_ibput##BITS##_on_stream, \
                  ishmemx_ibget##BITS##_on_stream, ishmemx_iput##BITS##_work_group, ishmemx_iget##BITS##_work_group, \
                  ishmemx_ibput##BITS##_work_group, ishmemx_ibget##BITS##_work_group)                           \
    };
KIND_TYPED(float, float)
KIND_TYPED(double, double)
KIND_TYPED(uint8, uint8_t)
KIND_TYPED(uint16, uint16_t)
KIND_TYPED(uint32, uint32_t)
KIND_TYPED(uint64, uint64_t)
KIND_SIZED(8)
KIND_SIZED(16)
KIND_SIZED(32)
KIND_SIZED(64)
KIND_SIZED(128)

__host__ __device__ inline size_t dest_off(const Call &c, size_t esz, size_t slot_b)
{
    return (size_t) c.slot * slot_b + kGuard + (size_t) c.doe * esz;
}
__host__ __device__ inline size_t src_off(const Call &c, size_t esz, size_t slot_b)
{
    return (size_t) c.slot * slot_b + kGuard + (size_t) c.soe * esz;
}

// G: 0 = one 256-thread block over all calls, 1 = one 64-lane tile over all calls, 2 = one call per
// thread, 3 = kSlices workgroups, each moving its own range of every call's blocks.
template <typename K, int G, bool PUT>
__global__ void strided_kernel(char *db, const char *sb, size_t slot_b, int pe)
{
    if constexpr (G == 2) {
        const int c = (int) (blockIdx.x * blockDim.x + threadIdx.x);
        if (c >= ncalls()) return;
        const Call cl = call_of(c);
        K::template thread<PUT>(db + dest_off(cl, K::esz, slot_b), sb + src_off(cl, K::esz, slot_b), cl, pe);
    } else {
        for (int c = 0; c < ncalls(); ++c) {
            const Call cl = call_of(c);
            size_t first = 0, n = cl.nblocks;
            if constexpr (G == 3) {
                first = cl.nblocks * blockIdx.x / kSlices;
                n = cl.nblocks * (blockIdx.x + 1) / kSlices - first;
            }
            char *d = db + dest_off(cl, K::esz, slot_b) + first * (size_t) cl.dst * K::esz;
            const char *s = sb + src_off(cl, K::esz, slot_b) + first * (size_t) cl.sst * K::esz;
            if constexpr (G == 1) {
                auto wave = cg::tiled_partition<64>(cg::this_thread_block());
                K::template group<PUT>(d, s, cl, n, pe, wave);
            } else {
                auto grp = cg::this_thread_block();
                K::template group<PUT>(d, s, cl, n, pe, grp);
            }
        }
    }
}

static void fill_words(uint8_t *out, size_t tag, int f, int t, size_t nbytes)
{
    const uint64_t base = ((uint64_t) tag << 48) + ((uint64_t) (0x80 + f) << 40) + ((uint64_t) (0x80 + t) << 32);
    for (size_t k = 0; k * 8 < nbytes; ++k) {
        const uint64_t w = base + k;  // x86-64 and gfx950 are little-endian
        memcpy(out + k * 8, &w, nbytes - k * 8 < 8 ? nbytes - k * 8 : 8);
    }
}

struct Bufs {
    char *sb, *db;  // symmetric heap
    uint8_t *host;  // pinned: dest arena read back
    std::vector<uint8_t> src, peer_src, want;
};

template <typename K, bool PUT>
static void kind_dir(Bufs &b)
{
    const int pe = ishmem_my_pe(), npes = ishmem_n_pes(), nxt = (pe + 1) % npes, prv = (pe + npes - 1) % npes;
    const size_t slot_b = slot_bytes(K::esz), arena = arena_bytes(K::esz);
    b.src.assign(arena, 0);
    b.peer_src.assign(arena, 0);
    b.want.assign(arena, 0xA5);
    for (int s = 0; s < kSlots; ++s) {
        // put: this PE's source goes to nxt, its dest receives from prv.  get: this PE's source is read
        // by prv, its dest receives nxt's source.
        fill_words(b.src.data() + s * slot_b, (size_t) s + 1, pe, PUT ? nxt : prv, slot_b);
        fill_words(b.peer_src.data() + s * slot_b, (size_t) s + 1, PUT ? prv : nxt, pe, slot_b);
    }
    for (int c = 0; c < ncalls(); ++c) {
        const Call cl = call_of(c);
        for (size_t blk = 0; blk < cl.nblocks; ++blk)
            memcpy(b.want.data() + dest_off(cl, K::esz, slot_b) + blk * (size_t) cl.dst * K::esz,
                   b.peer_src.data() + src_off(cl, K::esz, slot_b) + blk * (size_t) cl.sst * K::esz, cl.bsize * K::esz);
    }
    ishmem_barrier_all();  // no peer still reads the previous source
    (void) hipMemcpy(b.sb, b.src.data(), arena, hipMemcpyHostToDevice);
    for (int mode = 0; mode < kModes; ++mode) {
        ++cases;
        (void) hipMemset(b.db, 0xA5, arena);
        ishmem_barrier_all();  // every source and every cleared dest is in place
        int r = 0;
        if (mode <= kOnStream) {
            for (int c = 0; c < ncalls(); ++c) {
                const Call cl = call_of(c);
                void *d = b.db + dest_off(cl, K::esz, slot_b);
                const void *s = b.sb + src_off(cl, K::esz, slot_b);
                if (mode == kHost) K::host(PUT, d, s, cl, nxt);
                else r |= K::on_stream(PUT, d, s, cl, nxt, 0);
            }
        } else if (mode == kBlock) {
            hipLaunchKernelGGL((strided_kernel<K, 0, PUT>), dim3(1), dim3(256), 0, 0, b.db, b.sb, slot_b, nxt);
        } else if (mode == kWave) {
            hipLaunchKernelGGL((strided_kernel<K, 1, PUT>), dim3(1), dim3(64), 0, 0, b.db, b.sb, slot_b, nxt);
        } else if (mode == kThread) {
            hipLaunchKernelGGL((strided_kernel<K, 2, PUT>), dim3(1), dim3(64), 0, 0, b.db, b.sb, slot_b, nxt);
        } else {
            hipLaunchKernelGGL((strided_kernel<K, 3, PUT>), dim3(kSlices), dim3(256), 0, 0, b.db, b.sb, slot_b, nxt);
        }
        const hipError_t e = hipDeviceSynchronize();
        ishmem_barrier_all();  // every PE's transfers are complete
        (void) hipMemcpy(b.host, b.db, arena, hipMemcpyDeviceToHost);
        size_t bad = 0, first = 0;
        if (memcmp(b.host, b.want.data(), arena) != 0)
            for (size_t i = 0; i < arena; ++i)
                if (b.host[i] != b.want[i] && bad++ == 0) first = i;
        if (r != 0 || e != hipSuccess || bad) {
            if (++errors <= 16)
                printf("[%d] FAIL %s %s mode %s: rc %d hip %d, %zu bytes differ, first in slot %zu at %ld %s\n", pe, K::name(),
                       PUT ? "put" : "get", kModeName[mode], r, (int) e, bad, first / slot_b,
                       (long) (first % slot_b) - (long) kGuard, r ? ishmemi_c_last_error() : "");
        }
    }
}

template <typename K>
static void kind_tests(Bufs &b)
{
    kind_dir<K, true>(b);
    kind_dir<K, false>(b);
}

int main()
{
    if (ishmemi_c_init() != 0) {
        printf("init failed: %s\n", ishmemi_c_last_error());
        return 2;
    }
    const int pe = ishmem_my_pe(), npes = ishmem_n_pes();
    const size_t arena = arena_bytes(16);
    Bufs b;
    b.sb = (char *) ishmem_align(256, arena);
    b.db = (char *) ishmem_align(256, arena);
    if (!b.sb || !b.db || hipHostMalloc((void **) &b.host, arena, 0) != hipSuccess) {
        printf("[%d] allocation failed\n", pe);
        return 2;
    }
    // Every call stays inside its slot.
    for (int c = 0; c < ncalls(); ++c) {
        const Call cl = call_of(c);
        const size_t de = (size_t) cl.doe + (cl.nblocks - 1) * (size_t) cl.dst + cl.bsize;
        const size_t se = (size_t) cl.soe + (cl.nblocks - 1) * (size_t) cl.sst + cl.bsize;
        if (de > kSlotElems || se > kSlotElems || cl.slot >= kSlots) {
            printf("[%d] call %d leaves its slot\n", pe, c);
            return 2;
        }
    }
    kind_tests<K_float>(b);
    kind_tests<K_double>(b);
    kind_tests<K_uint8>(b);
    kind_tests<K_uint16>(b);
    kind_tests<K_uint32>(b);
    kind_tests<K_uint64>(b);
    kind_tests<K_8>(b);
    kind_tests<K_16>(b);
    kind_tests<K_32>(b);
    kind_tests<K_64>(b);
    kind_tests<K_128>(b);

    ishmem_barrier_all();
    errors += ishmemi_c_error_count();
    (void) hipHostFree(b.host);
    ishmem_free(b.db);
    ishmem_free(b.sb);
    ishmem_finalize();
    printf("[%d] %ld cases on %d PEs\n", pe, cases, npes);
    printf("%s errors %d\n", errors ? "FAIL" : "PASS", errors);
    return errors ? 1 : 0;
}
