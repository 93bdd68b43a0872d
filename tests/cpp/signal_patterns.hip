// put with signal, wait_until and test from inside kernels, through the C++ names of include/ishmem.h,
// include/ishmemx.h and include/ishmemx_device.h (the reference's test/unit/put_signal*.cpp,
// signal_wait_until*.cpp, wait_until*.cpp and test*.cpp shapes).
//   Ping-pong: ONE kernel per PE, 8 rounds, payloads of 256 B and 64 KiB.  In round r the payload goes
//   once round the ring (with two PEs: there and back): PE 0 puts to its successor with the signal
//   (SET, r); every other PE waits until its signal word equals r, EVERY thread checks dest with plain
//   loads, and the PE puts its own round-r payload on; PE 0 ends the round by waiting and checking.
//   Each PE reads all of dest four times with plain loads at the start of the round, so the check
//   meets warm, stale lines (a consumer with cold caches proves nothing).  Nothing but the signal
//   orders a put against the check.  Run by a 256-thread block, a 64-lane tile and one work-item.
//   wait_until / test: ishmem_<TN>_test is 0 before and 1 after the predecessor's device
//   ishmem_<TN>_p, ishmem_<TN>_wait_until returns after it; int, uint64 and ptrdiff, all six
//   comparisons, values for which a comparison in the wrong signedness or of the low half alone
//   answers differently; by one work-item and by a thread block.
//   Fan-in: every PE but 0 puts its slice into PE 0 and adds 1 to one signal; PE 0 waits for npes - 1.
//   Host: the blocking and on-stream C++ names, once each.
//   SIGNAL_PATTERNS_BOUNDED=1: the program sets ISHMEM_TIMEOUT_MS=300 and waits, in a kernel, for a
//   word nobody writes: the waits return, signal_wait_until with the last value read, and the error
//   shows in ishmemi_c_error_count().
// Launch: ISHMEM_PE=<pe> ISHMEM_NPES=<n> ISHMEM_DEVICE=0 ISHMEM_BOOTSTRAP_KEY=<k> ./signal_patterns
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

constexpr int kRounds = 8, kWarmReads = 4;
enum Mode { kBlock = 0, kTile = 1, kThread = 2 };
static const char *const kModeName[3] = {"work_group", "wave_tile", "thread"};

__host__ __device__ inline uint32_t word_of(int round, int pe, uint32_t i)
{
    return (uint32_t) (round + 1) * 0x01000193u ^ ((uint32_t) pe << 24) ^ i;
}

template <int MODE>
__device__ inline void send(uint32_t *dest, const uint32_t *src, size_t nwords, uint64_t *sig, uint64_t value, int pe)
{
    if constexpr (MODE == kBlock) {
        ishmemx_putmem_signal_work_group(dest, src, nwords * 4, sig, value, ISHMEM_SIGNAL_SET, pe, cg::this_thread_block());
    } else if constexpr (MODE == kTile) {
        ishmemx_uint32_put_signal_work_group(dest, src, nwords, sig, value, ISHMEM_SIGNAL_SET, pe,
                                             cg::tiled_partition<64>(cg::this_thread_block()));
    } else {
        ishmem_int_put_signal((int *) dest, (const int *) src, nwords, sig, value, ISHMEM_SIGNAL_SET, pe);
    }
}

template <int MODE>
__device__ inline uint64_t wait_for(uint64_t *sig, uint64_t value)
{
    if constexpr (MODE == kBlock) return ishmemx_signal_wait_until_work_group(sig, ISHMEM_CMP_EQ, value, cg::this_thread_block());
    else if constexpr (MODE == kTile)
        return ishmemx_signal_wait_until_work_group(sig, ISHMEM_CMP_EQ, value, cg::tiled_partition<64>(cg::this_thread_block()));
    else return ishmem_signal_wait_until(sig, ISHMEM_CMP_EQ, value);
}

template <int MODE>
__global__ void pingpong_kernel(uint32_t *dest, uint32_t *src, uint64_t *sig, size_t nwords, int nxt, int prv, int me, int *bad,
                                uint32_t *sink)
{
    uint32_t acc = 0;
    for (int round = 1; round <= kRounds; ++round) {
        // plain reads of dest: this CU's L1 and this XCD's L2 now hold lines of an earlier round
        for (int w = 0; w < kWarmReads; ++w) {
            for (size_t i = threadIdx.x; i < nwords; i += blockDim.x) acc += dest[i];
            asm volatile("" ::: "memory");  // four separate passes of loads
        }
        for (int half = 0; half < 2; ++half) {
            if ((half == 0) == (me != 0)) {
                // receive: the signal alone says the payload is there; then every thread checks
                const uint64_t v = wait_for<MODE>(sig, (uint64_t) round);
                int wrong = v != (uint64_t) round;
                for (size_t i = threadIdx.x; i < nwords; i += blockDim.x) wrong += dest[i] != word_of(round, prv, (uint32_t) i);
                if (wrong) atomicAdd(bad, wrong);
            }
            if (half == 0) {
                // send this PE's round-r payload on (PE 0 starts the round, the others pass it on)
                for (size_t i = threadIdx.x; i < nwords; i += blockDim.x) src[i] = word_of(round, me, (uint32_t) i);
                __syncthreads();
                send<MODE>(dest, src, nwords, sig, (uint64_t) round, nxt);
            }
        }
    }
    if (acc == 0x12345678u) *sink = acc;  // keeps the warm reads
}

// ---- wait_until / test against the predecessor's ishmem_<TN>_p ----------------------------------
struct Flip {
    int cmp;
    long long before, cval, after;
};
// lo / mid / hi per type: int -1 / 0 / 1; uint64 7 / 7 + 2^32 / 7 + 2^63; ptrdiff 7 - 2^32 / 7 / 7 + 2^32.
static std::vector<Flip> flips(long long lo, long long mid, long long hi)
{
    return {{ISHMEM_CMP_EQ, lo, mid, mid}, {ISHMEM_CMP_NE, mid, mid, hi}, {ISHMEM_CMP_GT, mid, mid, hi},
            {ISHMEM_CMP_GE, lo, mid, mid}, {ISHMEM_CMP_LT, mid, mid, lo}, {ISHMEM_CMP_LE, hi, mid, mid}};
}

#define WAITTEST_KERNEL(TN, TYPE)                                                                                 \
    template <bool WG>                                                                                          \
    __global__ void waittest_##TN##_kernel(TYPE *ivar, int cmp, TYPE cval, TYPE after, int nxt, int *bad)        \
    {                                                                                                           \
        auto grp = cg::this_thread_block();                                                                     \
        int wrong = 0;                                                                                          \
        if constexpr (WG) {                                                                                     \
            wrong += ishmemx_##TN##_test_work_group(ivar, cmp, cval, grp) != 0;                                 \
            ishmemx_barrier_all_work_group(grp); /* every PE has tested before any variable flips */           \
            if (grp.thread_rank() == 0) ishmem_##TN##_p(ivar, after, nxt);                                      \
            ishmemx_##TN##_wait_until_work_group(ivar, cmp, cval, grp);                                         \
            wrong += ishmemx_##TN##_test_work_group(ivar, cmp, cval, grp) != 1;                                 \
            wrong += *ivar != after; /* a plain load after the wait, by every thread */                         \
        } else {                                                                                                \
            wrong += ishmem_##TN##_test(ivar, cmp, cval) != 0;                                                  \
            ishmem_barrier_all();                                                                               \
            ishmem_##TN##_p(ivar, after, nxt);                                                                  \
            ishmem_##TN##_wait_until(ivar, cmp, cval);                                                          \
            wrong += ishmem_##TN##_test(ivar, cmp, cval) != 1;                                                  \
            wrong += *ivar != after;                                                                            \
        }                                                                                                       \
        if (wrong) atomicAdd(bad, wrong);                                                                       \
    }                                                                                                           \
    static void waittest_##TN(TYPE *ivar, int *bad, int pe, int nxt, const std::vector<Flip> &fl)                \
    {                                                                                                           \
        for (const Flip &f : fl)                                                                                \
            for (int wg = 0; wg < 2; ++wg) {                                                                    \
                ++cases;                                                                                        \
                const TYPE before = (TYPE) f.before;                                                            \
                bad[0] = 0;                                                                                     \
                (void) hipMemcpy(ivar, &before, sizeof(TYPE), hipMemcpyHostToDevice);                           \
                ishmem_barrier_all();                                                                           \
                if (wg) hipLaunchKernelGGL(waittest_##TN##_kernel<true>, dim3(1), dim3(128), 0, 0, ivar, f.cmp, \
                                           (TYPE) f.cval, (TYPE) f.after, nxt, bad);                            \
                else hipLaunchKernelGGL(waittest_##TN##_kernel<false>, dim3(1), dim3(1), 0, 0, ivar, f.cmp,     \
                                        (TYPE) f.cval, (TYPE) f.after, nxt, bad);                               \
                const hipError_t e = hipDeviceSynchronize();                                                    \
                if (e != hipSuccess || bad[0]) {                                                                \
                    ++errors;                                                                                   \
                    printf("[%d] FAIL " #TN " wait_until / test cmp %d %s: hip %d, %d wrong answers\n", pe, f.cmp, \
                           wg ? "work_group" : "thread", (int) e, bad[0]);                                      \
                }                                                                                               \
                ishmem_barrier_all();                                                                           \
            }                                                                                                   \
    }
WAITTEST_KERNEL(int, int)
WAITTEST_KERNEL(uint64, uint64_t)
WAITTEST_KERNEL(ptrdiff, ptrdiff_t)

// ---- fan-in with ADD ----------------------------------------------------------------------------
__global__ void fanin_kernel(uint32_t *dest, uint32_t *src, uint64_t *sig, size_t nwords, int me, int npes, int *bad)
{
    auto grp = cg::this_thread_block();
    if (me != 0) {
        for (size_t i = threadIdx.x; i < nwords; i += blockDim.x) src[i] = word_of(77, me, (uint32_t) i);
        __syncthreads();
        ishmemx_putmem_signal_work_group(dest + (size_t) me * nwords, src, nwords * 4, sig, 1, ISHMEM_SIGNAL_ADD, 0, grp);
        return;
    }
    const uint64_t v = ishmemx_signal_wait_until_work_group(sig, ISHMEM_CMP_EQ, (uint64_t) (npes - 1), grp);
    int wrong = v != (uint64_t) (npes - 1) || ishmem_signal_fetch(sig) != (uint64_t) (npes - 1);
    for (int f = 1; f < npes; ++f)
        for (size_t i = threadIdx.x; i < nwords; i += blockDim.x)
            wrong += dest[(size_t) f * nwords + i] != word_of(77, f, (uint32_t) i);
    if (wrong) atomicAdd(bad, wrong);
}

// ---- bounded waits ------------------------------------------------------------------------------
__global__ void bounded_kernel(uint64_t *sig, int *ivar, uint64_t *out)
{
    auto grp = cg::this_thread_block();
    out[0] = ishmemx_signal_wait_until_work_group(sig, ISHMEM_CMP_EQ, 99, grp);
    if (grp.thread_rank() == 0) {
        ishmem_int_wait_until(ivar, ISHMEM_CMP_GT, 1000);
        out[1] = (uint64_t) ishmem_int_test(ivar, ISHMEM_CMP_GT, 1000) + 10;
        ishmem_int_wait_until(ivar, 0, 1000);  // an invalid comparison returns at once
        out[2] = 1;
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
    uint64_t *w = (uint64_t *) ishmem_align(256, 256), *out = nullptr;
    if (!w || hipHostMalloc((void **) &out, 64, 0) != hipSuccess) return 2;
    const uint64_t init[2] = {3, 5};
    (void) hipMemcpy(w, init, sizeof(init), hipMemcpyHostToDevice);
    memset(out, 0, 64);
    const int before = ishmemi_c_error_count();
    hipLaunchKernelGGL(bounded_kernel, dim3(1), dim3(256), 0, 0, w, (int *) (w + 1), out);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess || out[0] != 3 || out[1] != 10 || out[2] != 1 || ishmemi_c_error_count() <= before) {
        ++errors;
        printf("[%d] FAIL bounded device waits: hip %d, signal_wait_until returned %llu, test %llu, done %llu, "
               "error count %d -> %d\n", pe, (int) e, (unsigned long long) out[0], (unsigned long long) out[1],
               (unsigned long long) out[2], before, ishmemi_c_error_count());
    }
    (void) hipHostFree(out);
    ishmem_free(w);
    ishmem_finalize();
    printf("%s errors %d\n", errors ? "FAIL" : "PASS", errors);
    return errors ? 1 : 0;
}

template <int MODE>
static void pingpong(uint32_t *db, uint32_t *sb, uint64_t *sig, int *bad, int pe, int nxt, int prv)
{
    for (size_t bytes : {(size_t) 256, (size_t) 65536}) {
        ++cases;
        bad[0] = 0;
        (void) hipMemset(db, 0xA5, bytes);
        (void) hipMemset(sig, 0, 8);
        ishmem_barrier_all();
        const int threads = MODE == kBlock ? 256 : MODE == kTile ? 64 : 1;
        hipLaunchKernelGGL(pingpong_kernel<MODE>, dim3(1), dim3(threads), 0, 0, db, sb, sig, bytes / 4, nxt, prv, pe, bad,
                           (uint32_t *) (bad + 1));
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess || bad[0]) {
            ++errors;
            printf("[%d] FAIL ping-pong %s %zu B: hip %d, %d stale or wrong words\n", pe, kModeName[MODE], bytes, (int) e,
                   bad[0]);
        }
        ishmem_barrier_all();
    }
}

int main()
{
    if (const char *b = getenv("SIGNAL_PATTERNS_BOUNDED"); b && *b == '1') return bounded_main();
    if (ishmemi_c_init() != 0) {
        printf("init failed: %s\n", ishmemi_c_last_error());
        return 2;
    }
    const int pe = ishmem_my_pe(), npes = ishmem_n_pes(), nxt = (pe + 1) % npes, prv = (pe + npes - 1) % npes;
    constexpr size_t kBytes = 65536;
    uint32_t *sb = (uint32_t *) ishmem_align(256, kBytes), *db = (uint32_t *) ishmem_align(256, kBytes * 16);
    uint64_t *words = (uint64_t *) ishmem_align(256, 256);
    int *bad = nullptr;
    if (!sb || !db || !words || hipHostMalloc((void **) &bad, 2 * sizeof(int), 0) != hipSuccess) {
        printf("[%d] allocation failed\n", pe);
        return 2;
    }
    pingpong<kBlock>(db, sb, words, bad, pe, nxt, prv);
    pingpong<kTile>(db, sb, words, bad, pe, nxt, prv);
    pingpong<kThread>(db, sb, words, bad, pe, nxt, prv);

    waittest_int((int *) (words + 1), bad, pe, nxt, flips(-1, 0, 1));
    waittest_uint64(words + 1, bad, pe, nxt, flips(7, 7 + (1ll << 32), (long long) (7ull + (1ull << 63))));
    waittest_ptrdiff((ptrdiff_t *) (words + 1), bad, pe, nxt, flips(7 - (1ll << 32), 7, 7 + (1ll << 32)));

    {  // fan-in
        ++cases;
        bad[0] = 0;
        (void) hipMemset(db, 0xA5, kBytes * 16);
        (void) hipMemset(words, 0, 8);
        ishmem_barrier_all();
        hipLaunchKernelGGL(fanin_kernel, dim3(1), dim3(256), 0, 0, db, sb, words, (size_t) 4099, pe, npes, bad);
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess || bad[0]) {
            ++errors;
            printf("[%d] FAIL fan-in: hip %d, %d wrong words\n", pe, (int) e, bad[0]);
        }
        ishmem_barrier_all();
    }

    {  // the host names: blocking, then on a stream
        hipStream_t st = nullptr;
        (void) hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        std::vector<uint32_t> h(1024), got(1024);
        for (int form = 0; form < 2; ++form) {
            ++cases;
            for (size_t i = 0; i < h.size(); ++i) h[i] = word_of(90 + form, pe, (uint32_t) i);
            (void) hipMemcpy(sb, h.data(), 4096, hipMemcpyHostToDevice);
            (void) hipMemset(db, 0xA5, 4096);
            (void) hipMemset(words, 0, 8);
            ishmem_barrier_all();
            uint64_t v = 0;
            if (form == 0) {
                ishmem_uint32_put_signal(db, sb, 1024, words, 5, ISHMEM_SIGNAL_SET, nxt);
                ishmemx_signal_add(words, 2, nxt);
                v = ishmem_signal_wait_until(words, ISHMEM_CMP_EQ, 7);
                if (ishmem_uint64_test(words, ISHMEM_CMP_GE, (uint64_t) 7) != 1 || ishmem_signal_fetch(words) != 7) v = 0;
            } else {
                int rc = ishmemx_putmem_signal_on_stream(db, sb, 4096, words, 7, ISHMEM_SIGNAL_SET, nxt, st);
                rc |= ishmemx_signal_wait_until_on_stream(words, ISHMEM_CMP_EQ, 7, words + 2, st);
                rc |= ishmemx_uint64_wait_until_on_stream(words, ISHMEM_CMP_NE, (uint64_t) 0, st);
                (void) hipStreamSynchronize(st);
                (void) hipMemcpy(&v, words + 2, 8, hipMemcpyDeviceToHost);
                if (rc) v = 0;
            }
            (void) hipMemcpy(got.data(), db, 4096, hipMemcpyDeviceToHost);
            int wrong = v != 7;
            for (size_t i = 0; i < got.size(); ++i) wrong += got[i] != word_of(90 + form, prv, (uint32_t) i);
            if (wrong) {
                ++errors;
                printf("[%d] FAIL host %s: %d wrong (value %llu) %s\n", pe, form ? "on_stream" : "blocking", wrong,
                       (unsigned long long) v, ishmemi_c_last_error());
            }
            ishmem_barrier_all();
        }
        (void) hipStreamDestroy(st);
    }

    ishmem_barrier_all();
    errors += ishmemi_c_error_count();
    (void) hipHostFree(bad);
    ishmem_free(words);
    ishmem_free(db);
    ishmem_free(sb);
    ishmem_finalize();
    printf("[%d] %ld cases on %d PEs\n", pe, cases, npes);
    printf("%s errors %d\n", errors ? "FAIL" : "PASS", errors);
    return errors ? 1 : 0;
}
