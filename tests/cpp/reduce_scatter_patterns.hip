// The reduce-scatter extension through the C++ names (include/ishmemx.h, include/ishmemx_device.h)
// with the reference tester's reduce patterns (restated in oracle/oracle.c, linked here as the
// CHECKER): member j's source is the tester's source pattern over p * n elements, and member k's dest
// must be elements [k n, (k + 1) n) of the tester's check pattern — the slice of what the reduce leaves.
// Modes: host blocking, host on-stream, work_group by a 1024-thread block, by a 64-lane tile, and the
// one-thread device call; on the world team and on the strided team of the even PEs; dest aligned
// (the device form's 16-B branch when the block is aligned too) and one element off (element-wise
// branch); and a kernel that alternates device reduce-scatters with a device reduce of the same team.
// dest sits between 64-byte guards of 0xA5; everything is checked on the host.
// Launch: ISHMEM_PE=<pe> ISHMEM_NPES=<n> ISHMEM_DEVICE=0 ISHMEM_BOOTSTRAP_KEY=<k> ./reduce_scatter_patterns
#include <hip/hip_cooperative_groups.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ishmem.h"
#include "ishmemx.h"

extern "C" {
#include "oracle.h"
}

namespace cg = cooperative_groups;

static int errors = 0;
static long cases = 0;

constexpr size_t kGuard = 64, kMaxOff = 16, kMaxElems = 16384;
enum Mode { kHost = 0, kOnStream = 1, kBlock = 2, kWave = 3, kThread = 4, kModes = 5 };
static const char *const kModeName[kModes] = {"host", "on_stream", "work_group", "wave_tile", "thread"};

struct Sum {
    static constexpr int op = OR_SUM, fam = PAT_ARITH;
    static constexpr const char *name = "sum";
    template <typename T> static int host(ishmem_team_t t, T *d, const T *s, size_t n) { return ishmemx_sum_reduce_scatter(t, d, s, n); }
    template <typename T> static int stream(ishmem_team_t t, T *d, const T *s, size_t n, int *ret) { return ishmemx_sum_reduce_scatter_on_stream(t, d, s, n, ret, (hipStream_t) 0); }
    template <typename T, typename G> __device__ static int group(int t, T *d, const T *s, size_t n, const G &g) { return ishmemx_sum_reduce_scatter_work_group(t, d, s, n, g); }
    template <typename T> __device__ static int one(int t, T *d, const T *s, size_t n) { return ishmemx_sum_reduce_scatter(t, d, s, n); }
};
struct Max {
    static constexpr int op = OR_MAX, fam = PAT_ARITH;
    static constexpr const char *name = "max";
    template <typename T> static int host(ishmem_team_t t, T *d, const T *s, size_t n) { return ishmemx_max_reduce_scatter(t, d, s, n); }
    template <typename T> static int stream(ishmem_team_t t, T *d, const T *s, size_t n, int *ret) { return ishmemx_max_reduce_scatter_on_stream(t, d, s, n, ret, (hipStream_t) 0); }
    template <typename T, typename G> __device__ static int group(int t, T *d, const T *s, size_t n, const G &g) { return ishmemx_max_reduce_scatter_work_group(t, d, s, n, g); }
    template <typename T> __device__ static int one(int t, T *d, const T *s, size_t n) { return ishmemx_max_reduce_scatter(t, d, s, n); }
};
struct Xor {
    static constexpr int op = OR_XOR, fam = PAT_XOR;
    static constexpr const char *name = "xor";
    template <typename T> static int host(ishmem_team_t t, T *d, const T *s, size_t n) { return ishmemx_xor_reduce_scatter(t, d, s, n); }
    template <typename T> static int stream(ishmem_team_t t, T *d, const T *s, size_t n, int *ret) { return ishmemx_xor_reduce_scatter_on_stream(t, d, s, n, ret, (hipStream_t) 0); }
    template <typename T, typename G> __device__ static int group(int t, T *d, const T *s, size_t n, const G &g) { return ishmemx_xor_reduce_scatter_work_group(t, d, s, n, g); }
    template <typename T> __device__ static int one(int t, T *d, const T *s, size_t n) { return ishmemx_xor_reduce_scatter(t, d, s, n); }
};

// G: 0 = the whole 1024-thread block, 1 = a 64-lane tile, 2 = one thread.
template <typename T, typename OP, int G>
__global__ void rs_kernel(int team, T *dest, const T *source, size_t n, int *rc)
{
    int r;
    if constexpr (G == 0) r = OP::group(team, dest, source, n, cg::this_thread_block());
    else if constexpr (G == 1) r = OP::group(team, dest, source, n, cg::tiled_partition<64>(cg::this_thread_block()));
    else r = OP::one(team, dest, source, n);
    if (threadIdx.x == 0) *rc = r;
}

// reduce-scatter, a reduce of the same team over the whole source into `all`, reduce-scatter again
// into `dest2`: the device collectives of one team share its epochs.
template <typename T, int G>
__global__ void alternate_kernel(int team, T *dest, T *dest2, T *all, const T *source, size_t n, size_t total, int *rc)
{
    int r = 0;
    if constexpr (G == 0) {
        auto grp = cg::this_thread_block();
        r |= ishmemx_sum_reduce_scatter_work_group(team, dest, source, n, grp);
        r |= ishmemx_sum_reduce_work_group(team, all, source, total, grp);
        r |= ishmemx_sum_reduce_scatter_work_group(team, dest2, source, n, grp);
    } else {
        auto wave = cg::tiled_partition<64>(cg::this_thread_block());
        r |= ishmemx_sum_reduce_scatter_work_group(team, dest, source, n, wave);
        r |= ishmemx_sum_reduce_work_group(team, all, source, total, wave);
        r |= ishmemx_sum_reduce_scatter_work_group(team, dest2, source, n, wave);
    }
    if (threadIdx.x == 0) *rc = r;
}

struct Bufs {
    char *sb, *db, *d2, *all;  // symmetric heap
    uint8_t *host;             // pinned: a dest region read back
    int *rc;                   // pinned, device-visible
};

struct Team {
    ishmem_team_t handle;
    int me, size;  // me < 0: this PE is no member (it only keeps step)
};

template <typename T>
static bool region_ok(const Bufs &b, const char *dev, const std::vector<T> &want, size_t doff, size_t *first)
{
    const size_t B = want.size() * sizeof(T), region = kGuard + doff + B + kGuard;
    (void) hipMemcpy(b.host, dev, region, hipMemcpyDeviceToHost);
    std::vector<uint8_t> w(region, 0xA5);
    memcpy(w.data() + kGuard + doff, want.data(), B);
    for (size_t i = 0; i < region; ++i)
        if (b.host[i] != w[i]) {
            *first = i;
            return false;
        }
    return true;
}

// One (type, op, n, dest offset) shape in every mode on team `t`.
template <typename T, typename OP>
static void shape(Bufs &b, const Team &t, size_t n, size_t soff, size_t doff)
{
    if (t.me < 0) return;
    const int pe = ishmem_my_pe(), dt = ishmemi_cxx::dtype_of<T>();
    const size_t total = (size_t) t.size * n, B = n * sizeof(T), region = kGuard + doff + B + kGuard;
    std::vector<T> src(total), chk(total);
    oracle_pattern_source(OP::fam, dt, t.me, total, src.data());
    oracle_pattern_check(OP::fam, OP::op, dt, t.size, total, chk.data());
    const std::vector<T> want(chk.begin() + (size_t) t.me * n, chk.begin() + (size_t) (t.me + 1) * n);
    // The previous shape's last collective has completed on this PE, so no member still reads sb.
    (void) hipMemcpy(b.sb + soff, src.data(), total * sizeof(T), hipMemcpyHostToDevice);
    T *dest = (T *) (b.db + kGuard + doff);
    const T *source = (const T *) (b.sb + soff);
    for (int mode = 0; mode < kModes; ++mode) {
        ++cases;
        (void) hipMemsetAsync(b.db, 0xA5, region, 0);
        *b.rc = -1;
        int r = 0;
        switch (mode) {
            case kHost:
                r = OP::host(t.handle, dest, source, n);
                *b.rc = 0;
                break;
            case kOnStream: r = OP::stream(t.handle, dest, source, n, b.rc); break;
            case kBlock:
                hipLaunchKernelGGL((rs_kernel<T, OP, 0>), dim3(1), dim3(1024), 0, 0, (int) t.handle, dest, source, n, b.rc);
                break;
            case kWave:
                hipLaunchKernelGGL((rs_kernel<T, OP, 1>), dim3(1), dim3(64), 0, 0, (int) t.handle, dest, source, n, b.rc);
                break;
            default:
                hipLaunchKernelGGL((rs_kernel<T, OP, 2>), dim3(1), dim3(1), 0, 0, (int) t.handle, dest, source, n, b.rc);
                break;
        }
        const hipError_t e = hipStreamSynchronize(0);
        size_t first = 0;
        const bool ok = region_ok(b, b.db, want, doff, &first);
        if (r != 0 || e != hipSuccess || *b.rc != 0 || !ok) {
            if (++errors <= 16)
                printf("[%d] FAIL %s reduce_scatter size %zu n %zu members %d soff %zu doff %zu mode %s: rc %d ret %d hip %d "
                       "first bad byte %ld %s\n", pe, OP::name, sizeof(T), n, t.size, soff, doff, kModeName[mode], r, *b.rc,
                       (int) e, ok ? -1L : (long) first - (long) (kGuard + doff), r ? ishmemi_c_last_error() : "");
        }
    }
}

template <typename T, typename OP>
static void type_tests(Bufs &b, const Team &t)
{
    for (size_t n : {(size_t) 1, (size_t) 3, (size_t) 4, (size_t) 64, (size_t) 1000, (size_t) 1027, kMaxElems}) {
        shape<T, OP>(b, t, n, 0, 0);          // aligned dest: the device forms' 16-B branch when n * size is a multiple of 16
        shape<T, OP>(b, t, n, 0, sizeof(T));  // dest one element off: their element-wise branch
    }
    shape<T, OP>(b, t, 1000, sizeof(T), 0);   // the source one element off
}

template <int G>
static void alternate(Bufs &b, const Team &t, size_t n)
{
    if (t.me < 0) return;
    const size_t total = (size_t) t.size * n;
    std::vector<int> src(total), chk(total);
    oracle_pattern_source(PAT_ARITH, OD_INT32, t.me, total, src.data());
    oracle_pattern_check(PAT_ARITH, OR_SUM, OD_INT32, t.size, total, chk.data());
    const std::vector<int> want(chk.begin() + (size_t) t.me * n, chk.begin() + (size_t) (t.me + 1) * n);
    (void) hipMemcpy(b.sb, src.data(), total * 4, hipMemcpyHostToDevice);
    for (char *p : {b.db, b.d2}) (void) hipMemset(p, 0xA5, 2 * kGuard + n * 4);
    (void) hipMemset(b.all, 0xA5, 2 * kGuard + total * 4);
    *b.rc = -1;
    ++cases;
    hipLaunchKernelGGL((alternate_kernel<int, G>), dim3(1), dim3(G == 0 ? 1024 : 64), 0, 0, (int) t.handle,
                       (int *) (b.db + kGuard), (int *) (b.d2 + kGuard), (int *) (b.all + kGuard), (const int *) b.sb, n, total,
                       b.rc);
    const hipError_t e = hipStreamSynchronize(0);
    size_t first = 0;
    const bool ok = region_ok(b, b.db, want, 0, &first) && region_ok(b, b.d2, want, 0, &first) &&
                    region_ok(b, b.all, chk, 0, &first);
    if (e != hipSuccess || *b.rc != 0 || !ok) {
        ++errors;
        printf("[%d] FAIL alternating reduce_scatter / reduce G %d n %zu members %d: ret %d hip %d\n", ishmem_my_pe(), G, n,
               t.size, *b.rc, (int) e);
    }
}

int main()
{
    if (ishmemi_c_init() != 0) {
        printf("init failed: %s\n", ishmemi_c_last_error());
        return 2;
    }
    const int pe = ishmem_my_pe(), npes = ishmem_n_pes();
    const size_t arena = (size_t) npes * kMaxElems * 8 + 2 * kGuard + 2 * kMaxOff + 256;
    Bufs b;
    b.sb = (char *) ishmem_align(256, arena);
    b.db = (char *) ishmem_align(256, arena);
    b.d2 = (char *) ishmem_align(256, arena);
    b.all = (char *) ishmem_align(256, arena);
    if (!b.sb || !b.db || !b.d2 || !b.all || hipHostMalloc((void **) &b.host, arena, 0) != hipSuccess ||
        hipHostMalloc((void **) &b.rc, sizeof(int), 0) != hipSuccess) {
        printf("[%d] allocation failed\n", pe);
        return 2;
    }
    const Team world{ISHMEM_TEAM_WORLD, pe, npes};
    Team even{ISHMEM_TEAM_INVALID, -1, (npes + 1) / 2};
    if (ishmem_team_split_strided(ISHMEM_TEAM_WORLD, 0, 2, even.size, nullptr, 0, &even.handle) != 0) {
        printf("[%d] team split failed: %s\n", pe, ishmemi_c_last_error());
        return 2;
    }
    if (pe % 2 == 0) even.me = pe / 2;
    for (const Team &t : {world, even}) {
        type_tests<int, Sum>(b, t);
        type_tests<float, Max>(b, t);
        type_tests<double, Sum>(b, t);
        type_tests<uint64_t, Xor>(b, t);
        type_tests<int16_t, Max>(b, t);
        alternate<0>(b, t, 1000);
        alternate<1>(b, t, 1027);
        ishmem_barrier_all();
    }
    errors += ishmemi_c_error_count();
    if (even.handle != ISHMEM_TEAM_INVALID) ishmem_team_destroy(even.handle);
    (void) hipHostFree(b.rc);
    (void) hipHostFree(b.host);
    ishmem_free(b.all);
    ishmem_free(b.d2);
    ishmem_free(b.db);
    ishmem_free(b.sb);
    ishmem_finalize();
    printf("[%d] %ld cases on %d PEs\n", pe, cases, npes);
    printf("%s errors %d\n", errors ? "FAIL" : "PASS", errors);
    return errors ? 1 : 0;
}
