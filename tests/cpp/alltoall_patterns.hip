// alltoall through the C++ names (include/ishmem.h, include/ishmemx.h, include/ishmemx_device.h) in
// the shape of the reference's test/unit/alltoall.cpp: aligned nelems = 1, 2, 4, ... 65,536 and the
// offset sweep (nelems 1..15, source and dest offsets 0..15 bytes in steps of the type size), for
// element sizes 1, 2, 4 and 8 bytes and for alltoallmem, in five modes: host blocking, on-stream,
// work_group by a 256-thread block, by a wavefront tile, and the single-thread device call.
// Source: word k of the block from member f to member t is the little-endian int64
// (nelems << 48) + ((0x80 + f) << 40) + ((0x80 + t) << 32) + k, truncated to the block's bytes
// (alltoall.cpp:47-90).  dest sits between 64-byte guards of 0xA5; everything is checked on the host.
// Launch: ISHMEM_PE=<pe> ISHMEM_NPES=<n> ISHMEM_DEVICE=0 ISHMEM_BOOTSTRAP_KEY=<k> ./alltoall_patterns
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

constexpr size_t kGuard = 64, kMaxOff = 16;
enum Mode { kHost = 0, kOnStream = 1, kBlock = 2, kWave = 3, kThread = 4, kModes = 5 };
static const char *const kModeName[kModes] = {"host", "on_stream", "work_group", "wave_tile", "thread"};

// G: 0 = the whole 256-thread block, 1 = a wavefront tile, 2 = one thread.  MEM: the byte forms.
template <typename T, int G, bool MEM>
__global__ void a2a_kernel(T *dest, const T *source, size_t n, int *rc)
{
    int r;
    if constexpr (G == 0) {
        auto grp = cg::this_thread_block();
        if constexpr (MEM) r = ishmemx_alltoallmem_work_group(dest, source, n, grp);
        else r = ishmemx_alltoall_work_group(dest, source, n, grp);
    } else if constexpr (G == 1) {
        auto wave = cg::tiled_partition<64>(cg::this_thread_block());
        if constexpr (MEM) r = ishmemx_alltoallmem_work_group(ISHMEM_TEAM_WORLD, dest, source, n, wave);
        else r = ishmemx_alltoall_work_group(ISHMEM_TEAM_WORLD, dest, source, n, wave);
    } else {
        if constexpr (MEM) r = ishmem_alltoallmem(dest, source, n);
        else r = ishmem_alltoall(dest, source, n);
    }
    if (threadIdx.x == 0) *rc = r;
}

static void fill_block(uint8_t *out, size_t nelems, int f, int t, size_t nbytes)
{
    const uint64_t base = ((uint64_t) nelems << 48) + ((uint64_t) (0x80 + f) << 40) + ((uint64_t) (0x80 + t) << 32);
    for (size_t k = 0; k * 8 < nbytes; ++k) {
        const uint64_t w = base + k;  // x86-64 and gfx950 are little-endian
        memcpy(out + k * 8, &w, nbytes - k * 8 < 8 ? nbytes - k * 8 : 8);
    }
}

struct Bufs {
    char *sb, *db;      // symmetric heap
    uint8_t *host;      // pinned: dest region read back
    int *rc;            // pinned, device-visible
    std::vector<uint8_t> src, want;
};

// One (type, nelems, offsets) shape in every mode.  The source is uploaded once; every mode gets a
// fresh 0xA5 dest region.
template <typename T, bool MEM>
static void shape(Bufs &b, size_t nelems, size_t soff, size_t doff)
{
    const int pe = ishmem_my_pe(), npes = ishmem_n_pes();
    const size_t B = nelems * sizeof(T), total = (size_t) npes * B;
    const size_t region = kGuard + kMaxOff + total + kGuard;
    b.src.resize(total);
    b.want.assign(region, 0xA5);
    for (int t = 0; t < npes; ++t) fill_block(b.src.data() + (size_t) t * B, nelems, pe, t, B);
    for (int j = 0; j < npes; ++j) fill_block(b.want.data() + kGuard + doff + (size_t) j * B, nelems, j, pe, B);
    // The previous shape's last collective has returned on this PE, so no peer still reads sb.
    (void) hipMemcpy(b.sb + soff, b.src.data(), total, hipMemcpyHostToDevice);
    T *dest = (T *) (b.db + kGuard + doff);
    const T *source = (const T *) (b.sb + soff);
    const size_t count = MEM ? B : nelems;
    for (int mode = 0; mode < kModes; ++mode) {
        ++cases;
        (void) hipMemsetAsync(b.db, 0xA5, region, 0);
        *b.rc = -1;
        int r = 0;
        switch (mode) {
            case kHost:
                if constexpr (MEM) r = ishmem_alltoallmem((void *) dest, (const void *) source, count);
                else r = ishmem_alltoall(dest, source, count);
                *b.rc = 0;
                break;
            case kOnStream:
                if constexpr (MEM) r = ishmemx_alltoallmem_on_stream((void *) dest, (const void *) source, count, b.rc, 0);
                else r = ishmemx_alltoall_on_stream(dest, source, count, b.rc, (hipStream_t) 0);
                break;
            case kBlock:
                hipLaunchKernelGGL((a2a_kernel<T, 0, MEM>), dim3(1), dim3(256), 0, 0, dest, source, count, b.rc);
                break;
            case kWave:
                hipLaunchKernelGGL((a2a_kernel<T, 1, MEM>), dim3(1), dim3(64), 0, 0, dest, source, count, b.rc);
                break;
            default:
                hipLaunchKernelGGL((a2a_kernel<T, 2, MEM>), dim3(1), dim3(1), 0, 0, dest, source, count, b.rc);
                break;
        }
        (void) hipMemcpyAsync(b.host, b.db, region, hipMemcpyDeviceToHost, 0);
        const hipError_t e = hipStreamSynchronize(0);
        size_t bad = 0, first = 0;
        for (size_t i = 0; i < region; ++i)
            if (b.host[i] != b.want[i] && bad++ == 0) first = i;
        if (r != 0 || e != hipSuccess || *b.rc != 0 || bad) {
            if (++errors <= 16)
                printf("[%d] FAIL alltoall%s size %zu nelems %zu soff %zu doff %zu mode %s: rc %d ret %d hip %d bad %zu "
                       "(first at %ld) %s\n", pe, MEM ? "mem" : "", sizeof(T), nelems, soff, doff, kModeName[mode], r,
                       *b.rc, (int) e, bad, (long) first - (long) (kGuard + doff), r ? ishmemi_c_last_error() : "");
        }
    }
}

template <typename T, bool MEM>
static void type_tests(Bufs &b)
{
    for (size_t n = 1; n <= 65536; n *= 2) shape<T, MEM>(b, n, 0, 0);
    for (size_t n = 1; n <= 15; ++n)
        for (size_t soff = 0; soff < 16; soff += sizeof(T))
            for (size_t doff = 0; doff < 16; doff += sizeof(T)) shape<T, MEM>(b, n, soff, doff);
}

int main()
{
    if (ishmemi_c_init() != 0) {
        printf("init failed: %s\n", ishmemi_c_last_error());
        return 2;
    }
    const int pe = ishmem_my_pe(), npes = ishmem_n_pes();
    const size_t arena = (size_t) npes * 65536 * 8 + 2 * kGuard + 2 * kMaxOff + 256;
    Bufs b;
    b.sb = (char *) ishmem_align(256, arena);
    b.db = (char *) ishmem_align(256, arena);
    if (!b.sb || !b.db || hipHostMalloc((void **) &b.host, arena, 0) != hipSuccess ||
        hipHostMalloc((void **) &b.rc, sizeof(int), 0) != hipSuccess) {
        printf("[%d] allocation failed\n", pe);
        return 2;
    }
    type_tests<uint8_t, false>(b);
    type_tests<uint16_t, false>(b);
    type_tests<uint32_t, false>(b);
    type_tests<uint64_t, false>(b);
    type_tests<uint8_t, true>(b);  // alltoallmem: byte counts, byte offsets
    ishmem_barrier_all();
    errors += ishmemi_c_error_count();
    (void) hipHostFree(b.rc);
    (void) hipHostFree(b.host);
    ishmem_free(b.db);
    ishmem_free(b.sb);
    ishmem_finalize();
    printf("[%d] %ld cases on %d PEs\n", pe, cases, npes);
    printf("%s errors %d\n", errors ? "FAIL" : "PASS", errors);
    return errors ? 1 : 0;
}
