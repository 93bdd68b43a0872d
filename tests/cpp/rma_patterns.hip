// put / get through the C++ names (include/ishmem.h, include/ishmemx.h, include/ishmemx_device.h) in
// the shape of the reference's test/unit/put.cpp, get.cpp, p.cpp and g.cpp.  Every PE puts to the
// next PE (me + 1) % npes, or gets from it.
//   Kinds: float, double, uint8, uint16, uint32, uint64, mem and the sized forms 8 .. 128.
//   Shapes: aligned nelems = 1, 2, 4, ... 16384, then the offset sweep: nelems 1..16 x source and
//   dest byte offsets 0..14 in steps of the element size.
//   Modes: host blocking, host _nbi + quiet, on-stream, work_group by a 256-thread block, by a
//   64-lane tile, single threads (one shape per thread, each with its own arguments), and a
//   multi-workgroup kernel in which each workgroup moves its own slice.
// Word k of a transfer of nelems elements from PE f to PE t is the little-endian int64
// (nelems << 48) + ((0x80 + f) << 40) + ((0x80 + t) << 32) + k, truncated to the transfer's bytes
// (ishmem_tester.h:1118-1149).  Every shape has its own slot of the dest arena, between guards of
// 0xA5; one mode moves all shapes between two barriers and the whole arena is compared on the host.
// p / g: N = 5 elements of all 23 typenames, from the host, a single thread and one thread per
// element.  Hand-off: inside ONE kernel per PE, 4 rounds of warm plain reads of dest, device barrier,
// ishmemx_putmem_work_group to the next PE + quiet, device barrier, plain reads that must see it.
// Launch: ISHMEM_PE=<pe> ISHMEM_NPES=<n> ISHMEM_DEVICE=0 ISHMEM_BOOTSTRAP_KEY=<k> ./rma_patterns
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

constexpr size_t kGuard = 64, kPow2 = 15, kMaxN = 16384, kSmallSlot = 512, kSlices = 8;
enum Mode { kHost = 0, kNbi = 1, kOnStream = 2, kBlock = 3, kWave = 4, kThread = 5, kMultiWg = 6, kModes = 7 };
static const char *const kModeName[kModes] = {"host", "nbi+quiet", "on_stream", "work_group", "wave_tile", "thread",
                                              "multi_wg"};

struct Shape {
    size_t n, soff, doff, slot;  // slot: byte offset of the shape's slot in both arenas
};

// Shape `i` of an element size: the aligned sizes first (big slots), then the sweep (small slots).
__host__ __device__ inline size_t sweep_steps(size_t esz) { return (14 / esz) + 1; }
__host__ __device__ inline size_t big_slot(size_t esz) { return kMaxN * esz + 256; }
__host__ __device__ inline size_t nshapes(size_t esz) { return kPow2 + 16 * sweep_steps(esz) * sweep_steps(esz); }
__host__ __device__ inline Shape shape_of(size_t i, size_t esz)
{
    if (i < kPow2) return Shape{(size_t) 1 << i, 0, 0, i * big_slot(esz)};
    const size_t k = i - kPow2, st = sweep_steps(esz);
    return Shape{k / (st * st) + 1, ((k / st) % st) * esz, (k % st) * esz, kPow2 * big_slot(esz) + k * kSmallSlot};
}
static size_t arena_bytes(size_t esz) { return kPow2 * big_slot(esz) + (nshapes(esz) - kPow2) * kSmallSlot; }

// ---- the names under test, one struct per kind ------------------------------------------------
#define KIND_BODY(ESZ, LABEL, PUT, GET, PUTNBI, GETNBI, XPUT, XGET, WPUT, WGET)                                   \
    static constexpr size_t esz = ESZ;                                                                          \
    static const char *name() { return LABEL; }                                                                 \
    static void put(void *d, const void *s, size_t n, int pe) { PUT((ET *) d, (const ET *) s, n, pe); }         \
    static void get(void *d, const void *s, size_t n, int pe) { GET((ET *) d, (const ET *) s, n, pe); }         \
    static void put_nbi(void *d, const void *s, size_t n, int pe) { PUTNBI((ET *) d, (const ET *) s, n, pe); }  \
    static void get_nbi(void *d, const void *s, size_t n, int pe) { GETNBI((ET *) d, (const ET *) s, n, pe); }  \
    static int put_os(void *d, const void *s, size_t n, int pe, hipStream_t st)                                 \
    {                                                                                                           \
        return XPUT((ET *) d, (const ET *) s, n, pe, st);                                                       \
    }                                                                                                           \
    static int get_os(void *d, const void *s, size_t n, int pe, hipStream_t st)                                 \
    {                                                                                                           \
        return XGET((ET *) d, (const ET *) s, n, pe, st);                                                       \
    }                                                                                                           \
    __device__ static void tput(void *d, const void *s, size_t n, int pe) { PUT((ET *) d, (const ET *) s, n, pe); } \
    __device__ static void tget(void *d, const void *s, size_t n, int pe) { GET((ET *) d, (const ET *) s, n, pe); } \
    template <typename G>                                                                                       \
    __device__ static void gput(void *d, const void *s, size_t n, int pe, const G &g)                           \
    {                                                                                                           \
        WPUT((ET *) d, (const ET *) s, n, pe, g);                                                               \
    }                                                                                                           \
    template <typename G>                                                                                       \
    __device__ static void gget(void *d, const void *s, size_t n, int pe, const G &g)                           \
    {                                                                                                           \
        WGET((ET *) d, (const ET *) s, n, pe, g);                                                               \
    }
#define KIND_TYPED(TN, TYPE)                                                                                    \
    struct K_##TN {                                                                                             \
        using ET = TYPE;                                                                                        \
        KIND_BODY(sizeof(TYPE), #TN, ishmem_##TN##_put, ishmem_##TN##_get, ishmem_##TN##_put_nbi,               \
                  ishmem_##TN##_get_nbi, ishmemx_##TN##_put_on_stream, ishmemx_##TN##_get_on_stream,            \
                  ishmemx_##TN##_put_work_group, ishmemx_##TN##_get_work_group)                                 \
    };
#define KIND_SIZED(SUFFIX, ESZ)                                                                                 \
    struct K_##SUFFIX {                                                                                         \
        using ET = void;                                                                                        \
        KIND_BODY(ESZ, #SUFFIX, ishmem_put##SUFFIX, ishmem_get##SUFFIX, ishmem_put##SUFFIX##_nbi,               \
                  ishmem_get##SUFFIX##_nbi, ishmemx_put##SUFFIX##_on_stream, ishmemx_get##SUFFIX##_on_stream,   \
                  ishmemx_put##SUFFIX##_work_group, ishmemx_get##SUFFIX##_work_group)                           \
    };
KIND_TYPED(float, float)
KIND_TYPED(double, double)
KIND_TYPED(uint8, uint8_t)
KIND_TYPED(uint16, uint16_t)
KIND_TYPED(uint32, uint32_t)
KIND_TYPED(uint64, uint64_t)
KIND_SIZED(mem, 1)
KIND_SIZED(8, 1)
KIND_SIZED(16, 2)
KIND_SIZED(32, 4)
KIND_SIZED(64, 8)
KIND_SIZED(128, 16)

// G: 0 = one 256-thread block over all shapes, 1 = one 64-lane tile over all shapes, 2 = one shape
// per thread, 3 = kSlices workgroups, each moving its own slice of every shape.
template <typename K, int G, bool PUT>
__global__ void rma_kernel(char *db, const char *sb, int pe)
{
    const size_t ns = nshapes(K::esz);
    if constexpr (G == 2) {
        const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= ns) return;
        const Shape s = shape_of(i, K::esz);
        char *d = db + s.slot + kGuard + s.doff;
        const char *src = sb + s.slot + kGuard + s.soff;
        if constexpr (PUT) K::tput(d, src, s.n, pe);
        else K::tget(d, src, s.n, pe);
    } else {
        for (size_t i = 0; i < ns; ++i) {
            const Shape s = shape_of(i, K::esz);
            size_t first = 0, n = s.n;
            if constexpr (G == 3) {
                first = s.n * blockIdx.x / kSlices;
                n = s.n * (blockIdx.x + 1) / kSlices - first;
            }
            char *d = db + s.slot + kGuard + s.doff + first * K::esz;
            const char *src = sb + s.slot + kGuard + s.soff + first * K::esz;
            if constexpr (G == 1) {
                auto wave = cg::tiled_partition<64>(cg::this_thread_block());
                if constexpr (PUT) K::gput(d, src, n, pe, wave);
                else K::gget(d, src, n, pe, wave);
            } else {
                auto grp = cg::this_thread_block();
                if constexpr (PUT) K::gput(d, src, n, pe, grp);
                else K::gget(d, src, n, pe, grp);
            }
        }
    }
}

static void fill_words(uint8_t *out, size_t nelems, int f, int t, size_t nbytes)
{
    const uint64_t base = ((uint64_t) nelems << 48) + ((uint64_t) (0x80 + f) << 40) + ((uint64_t) (0x80 + t) << 32);
    for (size_t k = 0; k * 8 < nbytes; ++k) {
        const uint64_t w = base + k;  // x86-64 and gfx950 are little-endian
        memcpy(out + k * 8, &w, nbytes - k * 8 < 8 ? nbytes - k * 8 : 8);
    }
}

struct Bufs {
    char *sb, *db;  // symmetric heap
    uint8_t *host;  // pinned: dest arena read back
    std::vector<uint8_t> src, want;
};

template <typename K, bool PUT>
static void kind_dir(Bufs &b)
{
    const int pe = ishmem_my_pe(), npes = ishmem_n_pes(), nxt = (pe + 1) % npes, prv = (pe + npes - 1) % npes;
    const size_t ns = nshapes(K::esz), arena = arena_bytes(K::esz);
    b.src.assign(arena, 0);
    b.want.assign(arena, 0xA5);
    for (size_t i = 0; i < ns; ++i) {
        const Shape s = shape_of(i, K::esz);
        // put: this PE's source goes to nxt, its dest receives from prv.  get: this PE's source is
        // read by prv, its dest receives nxt's source.
        fill_words(b.src.data() + s.slot + kGuard + s.soff, s.n, pe, PUT ? nxt : prv, s.n * K::esz);
        fill_words(b.want.data() + s.slot + kGuard + s.doff, s.n, PUT ? prv : nxt, pe, s.n * K::esz);
    }
    ishmem_barrier_all();  // no peer still reads the previous source
    (void) hipMemcpy(b.sb, b.src.data(), arena, hipMemcpyHostToDevice);
    for (int mode = 0; mode < kModes; ++mode) {
        ++cases;
        (void) hipMemset(b.db, 0xA5, arena);
        ishmem_barrier_all();  // every source and every cleared dest is in place
        int r = 0;
        if (mode <= kOnStream) {
            for (size_t i = 0; i < ns; ++i) {
                const Shape s = shape_of(i, K::esz);
                void *d = b.db + s.slot + kGuard + s.doff;
                const void *src = b.sb + s.slot + kGuard + s.soff;
                if (mode == kHost) PUT ? K::put(d, src, s.n, nxt) : K::get(d, src, s.n, nxt);
                else if (mode == kNbi) PUT ? K::put_nbi(d, src, s.n, nxt) : K::get_nbi(d, src, s.n, nxt);
                else r |= PUT ? K::put_os(d, src, s.n, nxt, 0) : K::get_os(d, src, s.n, nxt, 0);
            }
            if (mode == kNbi) ishmem_quiet();
        } else if (mode == kBlock) {
            hipLaunchKernelGGL((rma_kernel<K, 0, PUT>), dim3(1), dim3(256), 0, 0, b.db, b.sb, nxt);
        } else if (mode == kWave) {
            hipLaunchKernelGGL((rma_kernel<K, 1, PUT>), dim3(1), dim3(64), 0, 0, b.db, b.sb, nxt);
        } else if (mode == kThread) {
            hipLaunchKernelGGL((rma_kernel<K, 2, PUT>), dim3((unsigned) ((ns + 127) / 128)), dim3(128), 0, 0, b.db,
                               b.sb, nxt);
        } else {
            hipLaunchKernelGGL((rma_kernel<K, 3, PUT>), dim3(kSlices), dim3(256), 0, 0, b.db, b.sb, nxt);
        }
        const hipError_t e = hipDeviceSynchronize();
        ishmem_barrier_all();  // every PE's transfers are complete
        (void) hipMemcpy(b.host, b.db, arena, hipMemcpyDeviceToHost);
        size_t bad = 0, first = 0;
        if (memcmp(b.host, b.want.data(), arena) != 0)
            for (size_t i = 0; i < arena; ++i)
                if (b.host[i] != b.want[i] && bad++ == 0) first = i;
        if (r != 0 || e != hipSuccess || bad) {
            size_t si = 0;
            while (si + 1 < ns && shape_of(si + 1, K::esz).slot <= first) ++si;
            const Shape s = shape_of(si, K::esz);
            if (++errors <= 16)
                printf("[%d] FAIL %s %s mode %s: rc %d hip %d, %zu bytes differ, first in shape %zu (nelems %zu soff %zu "
                       "doff %zu) at %ld %s\n", pe, K::name(), PUT ? "put" : "get", kModeName[mode], r, (int) e, bad, si,
                       s.n, s.soff, s.doff, (long) first - (long) (s.slot + kGuard + s.doff), r ? ishmemi_c_last_error() : "");
        }
    }
}

template <typename K>
static void kind_tests(Bufs &b)
{
    kind_dir<K, true>(b);
    kind_dir<K, false>(b);
}

// ---- p / g (p.cpp, g.cpp: N = 5) ----------------------------------------------------------------
constexpr int kN = 5;
template <typename T>
__host__ __device__ inline T pg_value(int pe, int i, int salt)
{
    return (T) (pe * 16 + i + 1 + salt);
}
// mode 0: one thread moves all N; mode 1: one thread per element.
template <typename T, bool P>
__global__ void pg_kernel(T *remote, T *local, int pe, int me, int salt, int per_thread)
{
    const int t = threadIdx.x;
    for (int i = per_thread ? t : 0; i < (per_thread ? t + 1 : kN); ++i) {
        if (i >= kN) break;
        if constexpr (P) ishmem_p(remote + i, pg_value<T>(me, i, salt), pe);
        else local[i] = ishmem_g(remote + i, pe);
    }
}

template <typename T, typename PF, typename GF>
static void pg_test(Bufs &b, const char *tn, int salt, PF host_p, GF host_g)
{
    const int pe = ishmem_my_pe(), npes = ishmem_n_pes(), nxt = (pe + 1) % npes, prv = (pe + npes - 1) % npes;
    T *sym = (T *) (b.db + kGuard);  // the remote side, both for p (dest) and g (source)
    T *out = (T *) (b.sb + kGuard);  // g's local results (device memory)
    T got[kN], mine[kN];
    for (int mode = 0; mode < 3; ++mode) {
        for (int is_p = 1; is_p >= 0; --is_p) {
            ++cases;
            for (int i = 0; i < kN; ++i) mine[i] = pg_value<T>(pe, i, salt + mode);
            (void) hipMemset(b.db, 0xA5, 2 * kGuard + kN * sizeof(T));
            (void) hipMemset(b.sb, 0xA5, 2 * kGuard + kN * sizeof(T));
            if (!is_p) (void) hipMemcpy(sym, mine, sizeof(mine), hipMemcpyHostToDevice);
            ishmem_barrier_all();
            if (mode == 0) {
                for (int i = 0; i < kN; ++i) {
                    if (is_p) host_p(sym + i, mine[i], nxt);
                    else got[i] = host_g(sym + i, nxt);
                }
            } else if (is_p) {
                hipLaunchKernelGGL((pg_kernel<T, true>), dim3(1), dim3(mode == 1 ? 1 : kN), 0, 0, sym, out, nxt, pe,
                                   salt + mode, mode == 2);
            } else {
                hipLaunchKernelGGL((pg_kernel<T, false>), dim3(1), dim3(mode == 1 ? 1 : kN), 0, 0, sym, out, nxt, pe,
                                   salt + mode, mode == 2);
            }
            (void) hipDeviceSynchronize();
            ishmem_barrier_all();
            if (is_p) (void) hipMemcpy(got, sym, sizeof(got), hipMemcpyDeviceToHost);
            else if (mode != 0) (void) hipMemcpy(got, out, sizeof(got), hipMemcpyDeviceToHost);
            int bad = 0;
            for (int i = 0; i < kN; ++i) {
                const T want = pg_value<T>(is_p ? prv : nxt, i, salt + mode);
                bad += memcmp(&got[i], &want, sizeof(T)) != 0;
            }
            uint8_t guards[2 * kGuard + kN * sizeof(T)];
            (void) hipMemcpy(guards, b.db, sizeof(guards), hipMemcpyDeviceToHost);
            if (is_p)
                for (size_t i = 0; i < sizeof(guards); ++i)
                    if ((i < kGuard || i >= kGuard + kN * sizeof(T)) && guards[i] != 0xA5) ++bad;
            if (bad && ++errors <= 16)
                printf("[%d] FAIL %s_%s mode %d: %d wrong\n", pe, tn, is_p ? "p" : "g", mode, bad);
            ishmem_barrier_all();
        }
    }
}

#define PG_ONE(TN, TYPE, U1, U2)                                                                                \
    pg_test<TYPE>(b, #TN, salt++, [](TYPE *d, TYPE v, int pe) { ishmem_##TN##_p(d, v, pe); },                    \
                  [](const TYPE *s, int pe) { return ishmem_##TN##_g(s, pe); });

// The typed device names too, once each (the kernels above use the generic ishmem_p / ishmem_g).
#define PG_DEV_NAMES(TN, TYPE, U1, U2)                                                                          \
    ishmem_##TN##_p((TYPE *) sym + kN + 1, ishmem_##TN##_g((const TYPE *) sym + kN, pe), pe);
__global__ void pg_names_kernel(char *sym, int pe)
{
    ISHMEMI_CXX_ARITH_TYPES(PG_DEV_NAMES, _, _)
}

// ---- in-kernel hand-off -------------------------------------------------------------------------
__device__ inline uint32_t handoff_word(int round, int pe, uint32_t i)
{
    return (uint32_t) (round + 1) * 0x01000193u ^ ((uint32_t) pe << 24) ^ i;
}

__global__ void handoff_kernel(uint32_t *dest, uint32_t *src, size_t nwords, int nxt, int prv, int me, int *bad,
                               uint32_t *sink)
{
    auto grp = cg::this_thread_block();
    uint32_t acc = 0;
    for (int round = 0; round < 4; ++round) {
        // 1. plain reads of dest: this CU's L1 and this XCD's L2 now hold the old lines
        for (size_t i = threadIdx.x; i < nwords; i += blockDim.x) acc += dest[i];
        // 2. every PE has read; nobody is still checking the previous round
        ishmemx_barrier_all_work_group(grp);
        // 3. this round's payload, put to the next PE
        for (size_t i = threadIdx.x; i < nwords; i += blockDim.x) src[i] = handoff_word(round, me, (uint32_t) i);
        __syncthreads();
        ishmemx_putmem_work_group(dest, src, nwords * 4, nxt, grp);
        ishmemx_quiet_work_group(grp);
        // 4. every PE's put is complete
        ishmemx_barrier_all_work_group(grp);
        // 5. every thread reads dest with plain loads: the previous PE's words of this round
        int wrong = 0;
        for (size_t i = threadIdx.x; i < nwords; i += blockDim.x) wrong += dest[i] != handoff_word(round, prv, (uint32_t) i);
        if (wrong) atomicAdd(bad, wrong);
    }
    if (acc == 0x12345678u) *sink = acc;  // keeps the warm reads
}

int main()
{
    if (ishmemi_c_init() != 0) {
        printf("init failed: %s\n", ishmemi_c_last_error());
        return 2;
    }
    const int pe = ishmem_my_pe(), npes = ishmem_n_pes(), nxt = (pe + 1) % npes, prv = (pe + npes - 1) % npes;
    const size_t arena = arena_bytes(16) > arena_bytes(1) ? arena_bytes(16) : arena_bytes(1);
    Bufs b;
    b.sb = (char *) ishmem_align(256, arena);
    b.db = (char *) ishmem_align(256, arena);
    int *bad = nullptr;
    if (!b.sb || !b.db || hipHostMalloc((void **) &b.host, arena, 0) != hipSuccess ||
        hipHostMalloc((void **) &bad, 2 * sizeof(int), 0) != hipSuccess) {
        printf("[%d] allocation failed\n", pe);
        return 2;
    }
    kind_tests<K_float>(b);
    kind_tests<K_double>(b);
    kind_tests<K_uint8>(b);
    kind_tests<K_uint16>(b);
    kind_tests<K_uint32>(b);
    kind_tests<K_uint64>(b);
    kind_tests<K_mem>(b);
    kind_tests<K_8>(b);
    kind_tests<K_16>(b);
    kind_tests<K_32>(b);
    kind_tests<K_64>(b);
    kind_tests<K_128>(b);

    int salt = 0;
    ISHMEMI_CXX_ARITH_TYPES(PG_ONE, _, _)
    (void) hipMemset(b.db, 0, 1024);
    ishmem_barrier_all();
    hipLaunchKernelGGL(pg_names_kernel, dim3(1), dim3(1), 0, 0, b.db, nxt);
    if (hipDeviceSynchronize() != hipSuccess) ++errors;
    ishmem_barrier_all();

    for (size_t bytes : {(size_t) 256, (size_t) 65536}) {
        ++cases;
        bad[0] = 0;
        (void) hipMemset(b.db, 0xA5, bytes);
        ishmem_barrier_all();
        hipLaunchKernelGGL(handoff_kernel, dim3(1), dim3(256), 0, 0, (uint32_t *) b.db, (uint32_t *) b.sb, bytes / 4, nxt,
                           prv, pe, bad, (uint32_t *) (bad + 1));
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess || bad[0]) {
            ++errors;
            printf("[%d] FAIL hand-off %zu B: hip %d, %d stale or wrong words\n", pe, bytes, (int) e, bad[0]);
        }
        ishmem_barrier_all();
    }

    ishmem_barrier_all();
    errors += ishmemi_c_error_count();
    (void) hipHostFree(bad);
    (void) hipHostFree(b.host);
    ishmem_free(b.db);
    ishmem_free(b.sb);
    ishmem_finalize();
    printf("[%d] %ld cases on %d PEs\n", pe, cases, npes);
    printf("%s errors %d\n", errors ? "FAIL" : "PASS", errors);
    return errors ? 1 : 0;
}
