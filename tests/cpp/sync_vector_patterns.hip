// The vector waits and tests from inside kernels and from the host, through the C++ names of
// include/ishmem.h, include/ishmemx.h and include/ishmemx_device.h (the reference's
// test/unit/wait_until_{all,any,some}*.cpp and test_{all,any,some}*.cpp shapes).  DESIGN.md §3f.
//   Fan-in: ONE kernel per PE.  Every PE (PE 0 too) puts a payload with a signal into its own slot on
//   PE 0, one signal word per origin.  PE 0 consumes in a wait_until_some loop: every thread checks
//   each reported origin's payload with plain loads, the leader marks status, and the loop goes on
//   until all origins are done.  PE 0 reads all payload lines four times with plain loads first, so
//   the check meets warm, stale lines.  Nothing but the signal orders a put against the check.
//   wait_until_all: every PE writes all n variables of its successor with ishmem_uint64_p; the
//   successor waits for all of them and every thread then reads them with plain loads.
//   test_any: a polling loop until the one element the predecessor writes is reported.
//   Each of the three by a 256-thread block, a 64-lane tile and one work-item.
//   Host: the blocking and on-stream C++ names, once each, on local values.
//   SYNC_VECTOR_BOUNDED=1: the program sets ISHMEM_TIMEOUT_MS=300 and waits, in a kernel, on words
//   nobody writes: the waits return (any: SIZE_MAX, some: 0) and show in ishmemi_c_error_count().
// Launch: ISHMEM_PE=<pe> ISHMEM_NPES=<n> ISHMEM_DEVICE=0 ISHMEM_BOOTSTRAP_KEY=<k> ./sync_vector_patterns
#include <hip/hip_cooperative_groups.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ishmem.h"
#include "ishmemx.h"

namespace cg = cooperative_groups;

static int errors = 0;
static long cases = 0;

constexpr int kWarmReads = 4;
constexpr size_t kVars = 300;  // more than one 64-element sub-pass of a sweeping wave, not a multiple of it
enum Mode { kBlock = 0, kTile = 1, kThread = 2 };
static const char *const kModeName[3] = {"work_group", "wave_tile", "thread"};
static const int kModeThreads[3] = {256, 64, 1};

__host__ __device__ inline uint32_t word_of(int round, int pe, uint32_t i)
{
    return (uint32_t) (round + 1) * 0x01000193u ^ ((uint32_t) pe << 24) ^ i;
}

template <int MODE>
__device__ inline void group_sync()
{
    if constexpr (MODE == kBlock) __syncthreads();
    else if constexpr (MODE == kTile) __builtin_amdgcn_wave_barrier();
}

template <int MODE>
__device__ inline void send(uint32_t *dest, const uint32_t *src, size_t nwords, uint64_t *sig, uint64_t value, int pe)
{
    if constexpr (MODE == kBlock)
        ishmemx_putmem_signal_work_group(dest, src, nwords * 4, sig, value, ISHMEM_SIGNAL_SET, pe, cg::this_thread_block());
    else if constexpr (MODE == kTile)
        ishmemx_uint32_put_signal_work_group(dest, src, nwords, sig, value, ISHMEM_SIGNAL_SET, pe,
                                             cg::tiled_partition<64>(cg::this_thread_block()));
    else ishmem_uint32_put_signal(dest, src, nwords, sig, value, ISHMEM_SIGNAL_SET, pe);
}

template <int MODE>
__device__ inline size_t wait_some(uint64_t *sigs, size_t n, size_t *indices, const int *status, uint64_t value)
{
    if constexpr (MODE == kBlock)
        return ishmemx_uint64_wait_until_some_work_group(sigs, n, indices, status, ISHMEM_CMP_EQ, value, cg::this_thread_block());
    else if constexpr (MODE == kTile)
        return ishmemx_wait_until_some_work_group(sigs, n, indices, status, ISHMEM_CMP_EQ, value,
                                                  cg::tiled_partition<64>(cg::this_thread_block()));
    else return ishmem_uint64_wait_until_some(sigs, n, indices, status, ISHMEM_CMP_EQ, value);
}

template <int MODE>
__global__ void fanin_kernel(uint32_t *slots, uint32_t *src, uint64_t *sigs, size_t *indices, int *status, size_t nwords, int me,
                             int npes, int round, int *bad, uint32_t *sink)
{
    uint32_t acc = 0;
    if (me == 0) {
        // plain reads of every slot: this CU's L1 and this XCD's L2 now hold lines of the round before
        for (int w = 0; w < kWarmReads; ++w) {
            for (size_t i = threadIdx.x; i < nwords * (size_t) npes; i += blockDim.x) acc += slots[i];
            asm volatile("" ::: "memory");
        }
    }
    for (size_t i = threadIdx.x; i < nwords; i += blockDim.x) src[i] = word_of(round, me, (uint32_t) i);
    group_sync<MODE>();
    send<MODE>(slots + (size_t) me * nwords, src, nwords, sigs + me, (uint64_t) round, 0);
    if (me == 0) {
        int wrong = 0;
        size_t done = 0;
        while (done < (size_t) npes) {
            const size_t cnt = wait_some<MODE>(sigs, (size_t) npes, indices, status, (uint64_t) round);
            if (cnt == 0 || cnt > (size_t) npes - done) {  // a timeout, or more than is left
                wrong += 1000;
                break;
            }
            for (size_t k = 0; k < cnt; ++k) {
                const size_t f = indices[k];
                if (f >= (size_t) npes || status[f] || (k && indices[k - 1] >= f)) {
                    wrong += 100;
                    continue;
                }
                for (size_t i = threadIdx.x; i < nwords; i += blockDim.x) wrong += slots[f * nwords + i] != word_of(round, (int) f, (uint32_t) i);
            }
            group_sync<MODE>();  // every thread has read status and indices
            if (threadIdx.x == 0)
                for (size_t k = 0; k < cnt; ++k)
                    if (indices[k] < (size_t) npes) status[indices[k]] = 1;
            group_sync<MODE>();
            done += cnt;
        }
        if (wrong) atomicAdd(bad, wrong);
    }
    if (acc == 0x12345678u) *sink = acc;  // keeps the warm reads
}

template <int MODE>
__global__ void all_kernel(uint64_t *ivars, size_t n, int nxt, int round, int *bad, uint32_t *sink)
{
    uint32_t acc = 0;
    for (int w = 0; w < kWarmReads; ++w) {
        for (size_t i = threadIdx.x; i < n; i += blockDim.x) acc += (uint32_t) ivars[i];
        asm volatile("" ::: "memory");
    }
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) ishmem_uint64_p(ivars + i, (uint64_t) round, nxt);
    if constexpr (MODE == kBlock) ishmemx_uint64_wait_until_all_work_group(ivars, n, (const int *) nullptr, ISHMEM_CMP_EQ, (uint64_t) round, cg::this_thread_block());
    else if constexpr (MODE == kTile)
        ishmemx_wait_until_all_work_group(ivars, n, (const int *) nullptr, ISHMEM_CMP_EQ, (uint64_t) round,
                                          cg::tiled_partition<64>(cg::this_thread_block()));
    else ishmem_uint64_wait_until_all(ivars, n, nullptr, ISHMEM_CMP_EQ, (uint64_t) round);
    int wrong = 0;
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) wrong += ivars[i] != (uint64_t) round;  // plain loads, every thread
    if (wrong) atomicAdd(bad, wrong);
    if (acc == 0x12345678u) *sink = acc;
}

template <int MODE>
__global__ void test_any_kernel(long *ivars, const long *cvals, size_t n, size_t k, int nxt, int *bad)
{
    // ivars are all 0 and cvals[i] = i + 1: only element k, once written with k + 1, compares equal
    size_t r = SIZE_MAX;
    if constexpr (MODE == kBlock) r = ishmemx_long_test_any_vector_work_group(ivars, n, (const int *) nullptr, ISHMEM_CMP_EQ, cvals, cg::this_thread_block());
    else if constexpr (MODE == kTile)
        r = ishmemx_long_test_any_vector_work_group(ivars, n, (const int *) nullptr, ISHMEM_CMP_EQ, cvals,
                                                    cg::tiled_partition<64>(cg::this_thread_block()));
    else r = ishmem_long_test_any_vector(ivars, n, nullptr, ISHMEM_CMP_EQ, cvals);
    int wrong = r != SIZE_MAX;  // nobody has written yet: the barrier below comes first
    if constexpr (MODE == kBlock) ishmemx_barrier_all_work_group(cg::this_thread_block());
    else if (threadIdx.x == 0) ishmem_barrier_all();
    group_sync<MODE>();
    if (threadIdx.x == 0) ishmem_long_p(ivars + k, (long) k + 1, nxt);
    for (long spins = 0; r == SIZE_MAX && spins < (1l << 20); ++spins) {
        if constexpr (MODE == kBlock) r = ishmemx_long_test_any_vector_work_group(ivars, n, (const int *) nullptr, ISHMEM_CMP_EQ, cvals, cg::this_thread_block());
        else if constexpr (MODE == kTile)
            r = ishmemx_long_test_any_vector_work_group(ivars, n, (const int *) nullptr, ISHMEM_CMP_EQ, cvals,
                                                        cg::tiled_partition<64>(cg::this_thread_block()));
        else r = ishmem_long_test_any_vector(ivars, n, nullptr, ISHMEM_CMP_EQ, cvals);
    }
    wrong += r != k;
    wrong += ivars[k] != (long) k + 1;  // a plain load after the test that reported it
    if (wrong) atomicAdd(bad, wrong);
}

// ---- bounded waits ------------------------------------------------------------------------------
__global__ void bounded_kernel(uint64_t *ivars, size_t n, size_t *indices, uint64_t *out)
{
    auto grp = cg::this_thread_block();
    out[0] = ishmemx_uint64_wait_until_any_work_group(ivars, n, (const int *) nullptr, ISHMEM_CMP_EQ, (uint64_t) 99, grp);
    out[1] = ishmemx_uint64_wait_until_some_work_group(ivars, n, indices, (const int *) nullptr, ISHMEM_CMP_GT, (uint64_t) 99, grp) + 10;
    ishmemx_uint64_wait_until_all_work_group(ivars, n, (const int *) nullptr, ISHMEM_CMP_NE, (uint64_t) 3, grp);
    if (grp.thread_rank() == 0) {
        out[2] = ishmem_uint64_wait_until_any(ivars, n, nullptr, ISHMEM_CMP_LT, (uint64_t) 3);
        out[3] = (uint64_t) ishmem_uint64_test_all(ivars, n, nullptr, ISHMEM_CMP_EQ, (uint64_t) 3) + 20;
        out[4] = ishmem_uint64_wait_until_any(ivars, n, nullptr, 0, (uint64_t) 3);  // an invalid comparison returns at once
        out[5] = 1;
    }
}

static int bounded_main()
{
    setenv("ISHMEM_TIMEOUT_MS", "300", 1);
    if (ishmemi_c_init() != 0) {
        printf("init failed: %s\n", ishmemi_c_last_error());
        return 2;
    }
    const int pe = ishmem_my_pe();
    const size_t n = 70;
    uint64_t *w = (uint64_t *) ishmem_align(256, 1024), *out = nullptr;
    size_t *indices = nullptr;
    if (!w || hipHostMalloc((void **) &out, 64, 0) != hipSuccess || hipMalloc((void **) &indices, n * sizeof(size_t)) != hipSuccess)
        return 2;
    std::vector<uint64_t> init(n, 3);
    (void) hipMemcpy(w, init.data(), n * 8, hipMemcpyHostToDevice);
    memset(out, 0, 64);
    const int before = ishmemi_c_error_count();
    hipLaunchKernelGGL(bounded_kernel, dim3(1), dim3(256), 0, 0, w, n, indices, out);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess || out[0] != SIZE_MAX || out[1] != 10 || out[2] != SIZE_MAX || out[3] != 21 || out[4] != SIZE_MAX ||
        out[5] != 1 || ishmemi_c_error_count() <= before) {
        ++errors;
        printf("[%d] FAIL bounded device waits: hip %d, any %llu, some %llu, thread any %llu, test_all %llu, bad cmp %llu, "
               "done %llu, error count %d -> %d\n", pe, (int) e, (unsigned long long) out[0], (unsigned long long) out[1],
               (unsigned long long) out[2], (unsigned long long) out[3], (unsigned long long) out[4],
               (unsigned long long) out[5], before, ishmemi_c_error_count());
    }
    (void) hipHostFree(out);
    (void) hipFree(indices);
    ishmem_free(w);
    ishmem_finalize();
    printf("%s errors %d\n", errors ? "FAIL" : "PASS", errors);
    return errors ? 1 : 0;
}

static void finish_case(const char *what, int mode, int pe, int *bad)
{
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess || bad[0]) {
        ++errors;
        printf("[%d] FAIL %s %s: hip %d, %d stale, wrong or missing\n", pe, what, kModeName[mode], (int) e, bad[0]);
    }
    ishmem_barrier_all();
}

template <int MODE>
static void device_cases(uint32_t *slots, uint32_t *src, uint64_t *sigs, uint64_t *ivars, long *cvals, size_t *indices,
                         int *status, int *bad, int pe, int npes, int round)
{
    const int nxt = (pe + 1) % npes, threads = kModeThreads[MODE];
    const size_t nwords = MODE == kThread ? 64 : 4099;
    {  // fan-in into PE 0, consumed with wait_until_some
        ++cases;
        bad[0] = 0;
        (void) hipMemset(status, 0, sizeof(int) * (size_t) npes);
        ishmem_barrier_all();
        hipLaunchKernelGGL(fanin_kernel<MODE>, dim3(1), dim3(threads), 0, 0, slots, src, sigs, indices, status, nwords, pe, npes,
                           round, bad, (uint32_t *) (bad + 1));
        finish_case("fan-in wait_until_some", MODE, pe, bad);
    }
    {  // wait_until_all on what the predecessor writes
        ++cases;
        bad[0] = 0;
        ishmem_barrier_all();
        hipLaunchKernelGGL(all_kernel<MODE>, dim3(1), dim3(threads), 0, 0, ivars, kVars, nxt, round, bad, (uint32_t *) (bad + 1));
        finish_case("wait_until_all", MODE, pe, bad);
    }
    {  // a test_any polling loop
        ++cases;
        bad[0] = 0;
        (void) hipMemset(ivars, 0, kVars * 8);
        ishmem_barrier_all();
        hipLaunchKernelGGL(test_any_kernel<MODE>, dim3(1), dim3(threads), 0, 0, (long *) ivars, cvals, kVars,
                           (size_t) (MODE == kBlock ? kVars - 1 : MODE == kTile ? 64 : 7), nxt, bad);
        finish_case("test_any loop", MODE, pe, bad);
    }
}

#define EXPECT(cond)                                                                              \
    do {                                                                                          \
        ++cases;                                                                                  \
        if (!(cond)) {                                                                            \
            ++errors;                                                                             \
            printf("[%d] FAIL host %s (%s)\n", pe, #cond, ishmemi_c_last_error());                \
        }                                                                                         \
    } while (0)

static void host_names(int pe, int *ivars, int *dstatus, int *dcv, size_t *dindices, size_t *dret)
{
    // local values 0 .. 9; element 4 is excluded; compare GE 5 / element-wise EQ i
    const size_t n = 10;
    int vals[10], cv[10], status[10] = {0, 0, 0, 0, 1, 0, 0, 0, 0, 0};
    size_t idx[10];
    for (int i = 0; i < 10; ++i) vals[i] = cv[i] = i;
    (void) hipMemcpy(ivars, vals, sizeof(vals), hipMemcpyHostToDevice);
    (void) hipMemcpy(dstatus, status, sizeof(status), hipMemcpyHostToDevice);
    (void) hipMemcpy(dcv, cv, sizeof(cv), hipMemcpyHostToDevice);
    const int before = ishmemi_c_error_count();
    ishmem_int_wait_until_all(ivars, n, status, ISHMEM_CMP_GE, 0);
    ishmem_int_wait_until_all_vector(ivars, n, status, ISHMEM_CMP_EQ, cv);
    EXPECT(ishmem_int_test_all(ivars, n, status, ISHMEM_CMP_GE, 0) == 1 && ishmem_int_test_all(ivars, n, status, ISHMEM_CMP_GE, 5) == 0);
    EXPECT(ishmem_int_test_all_vector(ivars, n, status, ISHMEM_CMP_EQ, cv) == 1);
    const size_t a1 = ishmem_int_wait_until_any(ivars, n, status, ISHMEM_CMP_GE, 5);
    const size_t a2 = ishmem_int_test_any(ivars, n, status, ISHMEM_CMP_GE, 5);
    EXPECT(a1 >= 5 && a1 < n && a2 == (a1 == 9 ? 5 : a1 + 1));  // the scan starts behind the last index returned
    const size_t a3 = ishmem_int_wait_until_any_vector(ivars, n, status, ISHMEM_CMP_EQ, cv);  // every element matches
    const size_t behind = (a2 + 1) % n == 4 ? 5 : (a2 + 1) % n;                                // 4 is excluded
    EXPECT(a3 == behind);
    EXPECT(ishmem_int_test_any_vector(ivars, n, status, ISHMEM_CMP_LT, cv) == SIZE_MAX);
    EXPECT(ishmem_int_wait_until_some(ivars, n, idx, status, ISHMEM_CMP_LT, 6) == 5 && idx[0] == 0 && idx[3] == 3 && idx[4] == 5);
    EXPECT(ishmem_int_test_some(ivars, n, idx, status, ISHMEM_CMP_GT, 100) == 0);
    EXPECT(ishmem_int_wait_until_some_vector(ivars, n, idx, status, ISHMEM_CMP_GE, cv) == 9 && idx[4] == 5 && idx[8] == 9);
    EXPECT(ishmem_test_some_vector(ivars, n, idx, (const int *) nullptr, ISHMEM_CMP_EQ, (const int *) cv) == 10 && idx[9] == 9);
    hipStream_t st = nullptr;
    (void) hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    size_t got[3] = {77, 77, 77};
    int rc = ishmemx_int_wait_until_all_on_stream(ivars, n, dstatus, ISHMEM_CMP_GE, 0, st);
    rc |= ishmemx_int_wait_until_all_vector_on_stream(ivars, n, dstatus, ISHMEM_CMP_EQ, dcv, st);
    rc |= ishmemx_int_wait_until_any_on_stream(ivars, n, dstatus, ISHMEM_CMP_EQ, 7, dret, st);
    rc |= ishmemx_int_wait_until_any_vector_on_stream(ivars, n, (const int *) nullptr, ISHMEM_CMP_GE, dcv, dret + 1, st);
    rc |= ishmemx_int_wait_until_some_on_stream(ivars, n, dindices, dstatus, ISHMEM_CMP_GT, 7, dret + 2, st);
    (void) hipStreamSynchronize(st);
    (void) hipMemcpy(got, dret, sizeof(got), hipMemcpyDeviceToHost);
    (void) hipMemcpy(idx, dindices, 2 * sizeof(size_t), hipMemcpyDeviceToHost);
    EXPECT(rc == 0 && got[0] == 7 && got[1] == 8 && got[2] == 2 && idx[0] == 8 && idx[1] == 9);
    rc = ishmemx_wait_until_some_vector_on_stream(ivars, n, dindices, dstatus, ISHMEM_CMP_EQ, (const int *) dcv, dret, st,
                                                   (const hipEvent_t *) nullptr, 0, (hipEvent_t) nullptr);
    (void) hipStreamSynchronize(st);
    (void) hipMemcpy(got, dret, sizeof(size_t), hipMemcpyDeviceToHost);
    EXPECT(rc == 0 && got[0] == 9);
    (void) hipStreamDestroy(st);
    EXPECT(ishmemi_c_error_count() == before);
}

int main()
{
    if (const char *b = getenv("SYNC_VECTOR_BOUNDED"); b && *b == '1') return bounded_main();
    if (ishmemi_c_init() != 0) {
        printf("init failed: %s\n", ishmemi_c_last_error());
        return 2;
    }
    const int pe = ishmem_my_pe(), npes = ishmem_n_pes();
    constexpr size_t kSlotWords = 4099;
    uint32_t *src = (uint32_t *) ishmem_align(256, kSlotWords * 4), *slots = (uint32_t *) ishmem_align(256, kSlotWords * 4 * 16);
    uint64_t *sigs = (uint64_t *) ishmem_align(256, 256), *ivars = (uint64_t *) ishmem_align(256, kVars * 8);
    int *bad = nullptr, *status = nullptr;
    size_t *indices = nullptr;
    long *cvals = nullptr;
    if (!src || !slots || !sigs || !ivars || hipHostMalloc((void **) &bad, 2 * sizeof(int), 0) != hipSuccess ||
        hipMalloc((void **) &status, 64 * sizeof(int)) != hipSuccess || hipMalloc((void **) &indices, 64 * sizeof(size_t)) != hipSuccess ||
        hipMalloc((void **) &cvals, kVars * sizeof(long)) != hipSuccess) {
        printf("[%d] allocation failed\n", pe);
        return 2;
    }
    std::vector<long> cv(kVars);
    for (size_t i = 0; i < kVars; ++i) cv[i] = (long) i + 1;
    (void) hipMemcpy(cvals, cv.data(), kVars * sizeof(long), hipMemcpyHostToDevice);
    (void) hipMemset(slots, 0xA5, kSlotWords * 4 * 16);
    (void) hipMemset(sigs, 0, 256);
    (void) hipMemset(ivars, 0, kVars * 8);
    ishmem_barrier_all();
    for (int rep = 0; rep < 2; ++rep) {
        device_cases<kBlock>(slots, src, sigs, ivars, cvals, indices, status, bad, pe, npes, 3 * rep + 1);
        device_cases<kTile>(slots, src, sigs, ivars, cvals, indices, status, bad, pe, npes, 3 * rep + 2);
        device_cases<kThread>(slots, src, sigs, ivars, cvals, indices, status, bad, pe, npes, 3 * rep + 3);
    }
    host_names(pe, (int *) ivars, status, (int *) cvals, indices, indices + 32);

    ishmem_barrier_all();
    errors += ishmemi_c_error_count();
    (void) hipHostFree(bad);
    (void) hipFree(status);
    (void) hipFree(indices);
    (void) hipFree(cvals);
    ishmem_free(ivars);
    ishmem_free(sigs);
    ishmem_free(slots);
    ishmem_free(src);
    ishmem_finalize();
    printf("[%d] %ld cases on %d PEs\n", pe, cases, npes);
    printf("%s errors %d\n", errors ? "FAIL" : "PASS", errors);
    return errors ? 1 : 0;
}
