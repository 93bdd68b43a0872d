// Atomic memory operations from inside kernels, through the C++ names of include/ishmem.h and
// include/ishmemx_device.h (the reference's test/unit/atomic_*.cpp shapes).  DESIGN.md §3d.
//   Contended: 4 workgroups x 256 threads on every PE call ishmem_int_atomic_fetch_inc(ctr, 0); PE 0
//   sorts all 1024 p fetched values: 0 .. 1024 p - 1 each once, ctr == 1024 p (a wave-uniform address:
//   the compiler may fold a wave's adds into one atomic).  The same with
//   ishmem_uint64_atomic_fetch_add(.., 0x100000001, 0), and with lane i on word i % 8 of PE i % p
//   (addresses and PEs diverge inside a wave), every word checked the same way.
//   Bits: thread t < 21 of PE q ORs bit 21 q + t into a mask on PE 0 (the fetched value lacks the
//   bit; 21 p bits at the end), XORs it twice (the mask is restored), ANDs it away.
//   Lock: lane 0 of 8 workgroups per PE, 8 rounds: compare_swap(lock, 0, id) on PE 0, bounded spin;
//   two plain counters on PE 0 read with ishmem_g and written + 1 with ishmem_p; ishmem_quiet();
//   atomic_set(lock, 0).  Both counters end at 64 p.
//   Swap: float / double -0.0 and NaN payloads go round the ring with atomic_swap; atomic_fetch
//   returns the same bits.  _nbi: *fetch after ishmem_quiet().  The example's pattern: every thread
//   atomic_inc(dst_wait, next), the leader wait_until(dst_wait, GE, nthreads).  A bad pe returns T().
//   Host: a few of the host names, blocking and _nbi.
// No loop here spins unbounded: the lock's spin has an iteration cap that is reported as a failure.
// Launch: ISHMEM_PE=<pe> ISHMEM_NPES=<n> ISHMEM_DEVICE=0 ISHMEM_BOOTSTRAP_KEY=<k> ./amo_patterns
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ishmem.h"
#include "ishmemx.h"

static int errors = 0;
static long cases = 0;

constexpr int kGrid = 4, kBlock = 256, kThreads = kGrid * kBlock;  // 1024 work-items per PE
constexpr int kWords = 8;
constexpr int kLockGroups = 8, kLockRounds = 8, kLockSpinCap = 1 << 20;
constexpr uint64_t kStep = 0x100000001ull;
constexpr uint64_t kSentinel = 0x5EA15EA15EA15EA1ull;

#define FAIL(...)                                                                                                      \
    do {                                                                                                               \
        ++errors;                                                                                                      \
        printf(__VA_ARGS__);                                                                                           \
    } while (0)

// 0: int fetch_inc on one word of PE 0; 1: uint64 fetch_add(kStep) on one word of PE 0; 2: lane i adds 1
// to word i % 8 of PE i % p.
__global__ void contended_kernel(int mode, int *ictr, uint64_t *uctr, uint64_t *words, int npes, uint64_t *out)
{
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (mode == 0) out[gid] = (uint64_t) (uint32_t) ishmem_int_atomic_fetch_inc(ictr, 0);
    else if (mode == 1) out[gid] = ishmem_uint64_atomic_fetch_add(uctr, kStep, 0);
    else out[gid] = ishmem_uint64_atomic_fetch_add(words + gid % kWords, (uint64_t) 1, gid % npes);
}

// phase 0: fetch_or; 1: fetch_xor twice; 2: and with ~bit.
__global__ void bits_kernel(int phase, uint64_t *mask, int me, int *bad)
{
    const int t = threadIdx.x;
    if (t >= 21) return;
    const uint64_t bit = 1ull << (21 * me + t);
    if (phase == 0) {
        if (ishmem_uint64_atomic_fetch_or(mask, bit, 0) & bit) atomicAdd(bad, 1);  // nobody else sets this bit
    } else if (phase == 1) {
        const uint64_t a = ishmem_uint64_atomic_fetch_xor(mask, bit, 0);
        const uint64_t b = ishmem_atomic_fetch_xor<unsigned long>((unsigned long *) mask, (unsigned long) bit, 0);
        if (!(a & bit) || (b & bit)) atomicAdd(bad, 1);
    } else {
        ishmem_uint64_atomic_and(mask, ~bit, 0);
    }
}

__global__ void lock_kernel(int *lock, long *c0, long *c1, int me, int *bad)
{
    if (threadIdx.x != 0) return;
    const int id = 1 + me * kLockGroups + (int) blockIdx.x;
    for (int round = 0; round < kLockRounds; ++round) {
        bool mine = false;
        for (int spin = 0; spin < kLockSpinCap && !mine; ++spin) {
            mine = ishmem_int_atomic_compare_swap(lock, 0, id, 0) == 0;
            if (!mine) __builtin_amdgcn_s_sleep(8);
        }
        if (!mine) {  // reported, never a hang
            atomicAdd(bad, 1);
            return;
        }
        const long a = ishmem_long_g(c0, 0), b = ishmem_long_g(c1, 0);
        ishmem_long_p(c0, a + 1, 0);
        ishmem_long_p(c1, b + 1, 0);
        ishmem_quiet();  // the plain stores are in PE 0's memory before the lock is released
        ishmem_int_atomic_set(lock, 0, 0);
    }
}

__host__ __device__ inline uint32_t fbits(int q) { return q % 3 == 0 ? 0x80000000u : q % 3 == 1 ? 0x7FC12345u : 0xFFC54321u; }
__host__ __device__ inline uint64_t dbits(int q)
{
    return q % 3 == 0 ? 0x8000000000000000ull : q % 3 == 1 ? 0x7FF80000DEADBEEFull : 0xFFF8000012345678ull;
}

// phase 0: swap this PE's value into the next PE's words; phase 1: fetch this PE's own words.
__global__ void swap_kernel(int phase, float *fw, double *dw, int me, int nxt, uint64_t *out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (phase == 0) {
        out[0] = __float_as_uint(ishmem_float_atomic_swap(fw, __uint_as_float(fbits(me)), nxt));
        out[1] = (uint64_t) __double_as_longlong(ishmem_double_atomic_swap(dw, __longlong_as_double((long long) dbits(me)), nxt));
    } else {
        out[2] = __float_as_uint(ishmem_float_atomic_fetch(fw, me));
        out[3] = (uint64_t) __double_as_longlong(ishmem_atomic_fetch<double>(dw, me));
    }
}

// 64 threads: fetch_add_nbi on the next PE's counter, each into its own fetch word; thread 0 also a
// compare_swap_nbi that matches and a double fetch_nbi.  *fetch is read after ishmem_quiet().
__global__ void nbi_kernel(uint64_t *ctr, int *iw, double *dw, int nxt, uint64_t *fetch, uint64_t *out)
{
    const int t = threadIdx.x;
    ishmem_uint64_atomic_fetch_add_nbi(fetch + t, ctr, (uint64_t) 1, nxt);
    if (t == 0) {
        ishmem_int_atomic_compare_swap_nbi((int *) (fetch + 64), iw, 41, 42, nxt);
        ishmem_double_atomic_fetch_nbi((double *) (fetch + 65), dw, nxt);
    }
    ishmem_quiet();
    out[t] = fetch[t];
    if (t == 0) {
        out[64] = (uint64_t) (uint32_t) * (int *) (fetch + 64);
        out[65] = fetch[65];
    }
}

// The example's pattern.
__global__ void inc_wait_kernel(int *dst_wait, int nxt, int nthreads)
{
    ishmem_int_atomic_inc(dst_wait, nxt);
    if (threadIdx.x == 0) ishmem_int_wait_until(dst_wait, ISHMEM_CMP_GE, nthreads);
}

__global__ void bad_pe_kernel(int *iw, uint64_t *uw, int npes, uint64_t *fetch, uint64_t *out)
{
    if (threadIdx.x != 0) return;
    out[0] = (uint64_t) (uint32_t) ishmem_int_atomic_fetch_add(iw, 5, npes);
    out[1] = ishmem_uint64_atomic_swap(uw, (uint64_t) 9, -1);
    out[2] = (uint64_t) __double_as_longlong(ishmem_double_atomic_fetch((double *) uw, npes + 3));
    ishmem_int_atomic_inc(iw, npes);
    ishmem_uint64_atomic_xor(uw, ~0ull, -2);
    ishmem_uint64_atomic_fetch_or_nbi(fetch, uw, (uint64_t) 1, npes);
    ishmem_quiet();
    out[3] = fetch[0];
}

static bool sync_ok(const char *what, int pe)
{
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) {  // nothing more is started on a device that reported an error
        printf("[%d] FAIL %s: hip %d (%s)\nFAIL errors %d\n", pe, what, (int) e, hipGetErrorString(e), errors + 1);
        fflush(stdout);
        _Exit(1);
    }
    return true;
}

int main()
{
    if (ishmemi_c_init() != 0) {
        printf("init failed: %s\n", ishmemi_c_last_error());
        return 2;
    }
    const int pe = ishmem_my_pe(), npes = ishmem_n_pes(), nxt = (pe + 1) % npes, prv = (pe + npes - 1) % npes;
    // Symmetric: 64 words of 8 bytes for counters, locks and masks; the gathered fetched values on PE 0.
    uint64_t *w = (uint64_t *) ishmem_align(256, 64 * 8);
    uint64_t *gath = (uint64_t *) ishmem_align(256, (size_t) ISHMEMI_C_MAX_PES * kThreads * 8);
    uint64_t *out = nullptr, *fetch = nullptr;
    int *bad = nullptr;
    if (!w || !gath || hipMalloc((void **) &out, kThreads * 8) != hipSuccess || hipMalloc((void **) &fetch, 128 * 8) != hipSuccess ||
        hipHostMalloc((void **) &bad, sizeof(int), 0) != hipSuccess) {
        printf("[%d] allocation failed\n", pe);
        return 2;
    }
    std::vector<uint64_t> h((size_t) npes * kThreads), hw(64);
    auto gather = [&]() {  // every PE's out[] into row pe of PE 0's gath, then to PE 0's host
        ishmem_putmem(gath + (size_t) pe * kThreads, out, kThreads * 8, 0);
        ishmem_barrier_all();
        if (pe == 0) (void) hipMemcpy(h.data(), gath, h.size() * 8, hipMemcpyDeviceToHost);
    };
    auto my_words = [&]() { (void) hipMemcpy(hw.data(), w, 64 * 8, hipMemcpyDeviceToHost); };

    for (int mode = 0; mode < 3; ++mode) {  // contended
        ++cases;
        (void) hipMemset(w, 0, 64 * 8);
        ishmem_barrier_all();
        hipLaunchKernelGGL(contended_kernel, dim3(kGrid), dim3(kBlock), 0, 0, mode, (int *) w, w + 1, w + 8, npes, out);
        if (!sync_ok("contended", pe)) break;
        gather();
        my_words();
        if (mode < 2 && pe == 0) {
            const uint64_t step = mode == 0 ? 1 : kStep, total = (uint64_t) npes * kThreads;
            std::sort(h.begin(), h.end());
            size_t wrong = 0;
            for (size_t k = 0; k < h.size(); ++k) wrong += h[k] != k * step;
            const uint64_t fin = mode == 0 ? (uint64_t) (uint32_t) * (int *) hw.data() : hw[1];
            if (wrong || fin != total * step)
                FAIL("[0] FAIL contended mode %d: %zu fetched values out of place, final %llx\n", mode, wrong, (unsigned long long) fin);
        }
        if (mode == 2) {
            // word j of PE q is the target of every gid with gid % 8 == j and gid % p == q, on every PE
            for (int j = 0; j < kWords; ++j) {
                uint64_t cnt = 0;
                for (int g = 0; g < kThreads; ++g) cnt += g % kWords == j && g % npes == pe;
                if (hw[8 + j] != cnt * npes) FAIL("[%d] FAIL divergent: word %d is %llu, want %llu\n", pe, j, (unsigned long long) hw[8 + j], (unsigned long long) (cnt * npes));
            }
            if (pe == 0) {
                for (int q = 0; q < npes; ++q)
                    for (int j = 0; j < kWords; ++j) {
                        std::vector<uint64_t> v;
                        for (int o = 0; o < npes; ++o)
                            for (int g = 0; g < kThreads; ++g)
                                if (g % kWords == j && g % npes == q) v.push_back(h[(size_t) o * kThreads + g]);
                        std::sort(v.begin(), v.end());
                        size_t wrong = 0;
                        for (size_t k = 0; k < v.size(); ++k) wrong += v[k] != k;
                        if (wrong) FAIL("[0] FAIL divergent: PE %d word %d: %zu of %zu fetched values out of place\n", q, j, wrong, v.size());
                    }
            }
        }
        ishmem_barrier_all();
    }

    {  // bits
        (void) hipMemset(w, 0, 64 * 8);
        bad[0] = 0;
        ishmem_barrier_all();
        const uint64_t full = npes * 21 >= 64 ? ~0ull : (1ull << (21 * npes)) - 1;
        for (int phase = 0; phase < 3; ++phase) {
            ++cases;
            hipLaunchKernelGGL(bits_kernel, dim3(1), dim3(64), 0, 0, phase, w, pe, bad);
            if (!sync_ok("bits", pe)) break;
            ishmem_barrier_all();
            my_words();
            const uint64_t want = phase < 2 ? full : 0;
            if (pe == 0 && (hw[0] != want || __builtin_popcountll(hw[0]) != (phase < 2 ? 21 * npes : 0)))
                FAIL("[0] FAIL bits phase %d: mask %llx, want %llx\n", phase, (unsigned long long) hw[0], (unsigned long long) want);
            ishmem_barrier_all();
        }
        if (bad[0]) FAIL("[%d] FAIL bits: %d fetched values had the wrong bit\n", pe, bad[0]);
    }

    {  // lock
        ++cases;
        (void) hipMemset(w, 0, 64 * 8);
        bad[0] = 0;
        ishmem_barrier_all();
        hipLaunchKernelGGL(lock_kernel, dim3(kLockGroups), dim3(64), 0, 0, (int *) w, (long *) (w + 1), (long *) (w + 2), pe, bad);
        if (sync_ok("lock", pe)) {
            ishmem_barrier_all();
            my_words();
            const long want = (long) kLockGroups * kLockRounds * npes;
            if (bad[0]) FAIL("[%d] FAIL lock: %d lanes gave up after %d attempts\n", pe, bad[0], kLockSpinCap);
            if (pe == 0 && ((long) hw[1] != want || (long) hw[2] != want || (int) hw[0] != 0))
                FAIL("[0] FAIL lock: counters %ld %ld, want %ld; lock word %d\n", (long) hw[1], (long) hw[2], want, (int) hw[0]);
        }
        ishmem_barrier_all();
    }

    {  // swap ring, float and double as bits
        ++cases;
        const uint32_t finit = 0x3FC00000u + (uint32_t) pe;
        const uint64_t dinit = 0x3FF8000000000000ull + (uint64_t) pe;
        (void) hipMemcpy(w, &finit, 4, hipMemcpyHostToDevice);
        (void) hipMemcpy(w + 1, &dinit, 8, hipMemcpyHostToDevice);
        ishmem_barrier_all();
        hipLaunchKernelGGL(swap_kernel, dim3(1), dim3(64), 0, 0, 0, (float *) w, (double *) (w + 1), pe, nxt, out);
        if (sync_ok("swap", pe)) {
            ishmem_barrier_all();
            hipLaunchKernelGGL(swap_kernel, dim3(1), dim3(64), 0, 0, 1, (float *) w, (double *) (w + 1), pe, nxt, out);
            (void) sync_ok("fetch", pe);
            uint64_t o[4];
            (void) hipMemcpy(o, out, sizeof(o), hipMemcpyDeviceToHost);
            if (o[0] != 0x3FC00000u + (uint32_t) nxt || o[1] != 0x3FF8000000000000ull + (uint64_t) nxt)
                FAIL("[%d] FAIL swap: old values %llx %llx\n", pe, (unsigned long long) o[0], (unsigned long long) o[1]);
            if (o[2] != fbits(prv) || o[3] != dbits(prv))
                FAIL("[%d] FAIL swap: fetch returned %llx %llx, want %x %llx\n", pe, (unsigned long long) o[2], (unsigned long long) o[3], fbits(prv), (unsigned long long) dbits(prv));
        }
        ishmem_barrier_all();
    }

    {  // _nbi device forms
        ++cases;
        std::vector<uint64_t> f(128, kSentinel), o(66);
        const int i41 = 41;
        const uint64_t d = dbits(1);
        (void) hipMemset(w, 0, 64 * 8);
        (void) hipMemcpy(w + 1, &i41, 4, hipMemcpyHostToDevice);
        (void) hipMemcpy(w + 2, &d, 8, hipMemcpyHostToDevice);
        (void) hipMemcpy(fetch, f.data(), 128 * 8, hipMemcpyHostToDevice);
        ishmem_barrier_all();
        hipLaunchKernelGGL(nbi_kernel, dim3(1), dim3(64), 0, 0, w, (int *) (w + 1), (double *) (w + 2), nxt, fetch, out);
        if (sync_ok("nbi", pe)) {
            ishmem_barrier_all();
            (void) hipMemcpy(o.data(), out, 66 * 8, hipMemcpyDeviceToHost);
            (void) hipMemcpy(f.data(), fetch, 128 * 8, hipMemcpyDeviceToHost);
            my_words();
            std::sort(o.begin(), o.begin() + 64);
            size_t wrong = 0;
            for (size_t k = 0; k < 64; ++k) wrong += o[k] != k;
            if (wrong || hw[0] != 64) FAIL("[%d] FAIL nbi fetch_add: %zu values out of place, counter %llu\n", pe, wrong, (unsigned long long) hw[0]);
            if (o[64] != 41 || *(int *) &hw[1] != 42) FAIL("[%d] FAIL nbi compare_swap: fetched %llu, word %d\n", pe, (unsigned long long) o[64], *(int *) &hw[1]);
            if (o[65] != d) FAIL("[%d] FAIL nbi fetch double: %llx\n", pe, (unsigned long long) o[65]);
            if (f[66] != kSentinel) FAIL("[%d] FAIL nbi: wrote past the fetch words\n", pe);
        }
        ishmem_barrier_all();
    }

    {  // the example's pattern
        ++cases;
        (void) hipMemset(w, 0, 64 * 8);
        ishmem_barrier_all();
        hipLaunchKernelGGL(inc_wait_kernel, dim3(1), dim3(kBlock), 0, 0, (int *) w, nxt, kBlock);
        if (sync_ok("inc + wait_until", pe)) {
            my_words();
            if (*(int *) hw.data() != kBlock) FAIL("[%d] FAIL inc + wait_until: dst_wait %d, want %d\n", pe, *(int *) hw.data(), kBlock);
        }
        ishmem_barrier_all();
    }

    {  // a bad pe returns, and returns T()
        ++cases;
        uint64_t o[4], init[2] = {7, 0x1234};
        (void) hipMemcpy(w, init, 16, hipMemcpyHostToDevice);
        (void) hipMemcpy(fetch, &kSentinel, 8, hipMemcpyHostToDevice);
        ishmem_barrier_all();
        hipLaunchKernelGGL(bad_pe_kernel, dim3(1), dim3(64), 0, 0, (int *) w, w + 1, npes, fetch, out);
        if (sync_ok("bad pe", pe)) {
            (void) hipMemcpy(o, out, sizeof(o), hipMemcpyDeviceToHost);
            ishmem_barrier_all();
            my_words();
            if (o[0] || o[1] || o[2] || o[3] != kSentinel || hw[0] != 7 || hw[1] != 0x1234)
                FAIL("[%d] FAIL bad pe: returned %llx %llx %llx, fetch %llx, words %llx %llx\n", pe, (unsigned long long) o[0],
                     (unsigned long long) o[1], (unsigned long long) o[2], (unsigned long long) o[3], (unsigned long long) hw[0],
                     (unsigned long long) hw[1]);
        }
        ishmem_barrier_all();
    }

    {  // a few host names: blocking, and _nbi + quiet with the fetch word in device memory
        ++cases;
        (void) hipMemset(w, 0, 64 * 8);
        (void) hipMemcpy(fetch, &kSentinel, 8, hipMemcpyHostToDevice);
        ishmem_barrier_all();
        const int a = ishmem_int_atomic_fetch_add((int *) w, 5, nxt);
        ishmem_int32_atomic_xor((int32_t *) w, 0x0F, nxt);          // 5 ^ 15 = 10
        const long c = ishmem_atomic_compare_swap<long>((long *) (w + 1), 0L, -3L, nxt);
        ishmem_size_atomic_fetch_inc_nbi((size_t *) fetch, (size_t *) (w + 1), nxt);  // fetches -3, leaves -2
        ishmem_double_atomic_set((double *) (w + 2), -0.0, nxt);
        ishmem_quiet();
        const double z = ishmem_double_atomic_fetch((double *) (w + 2), nxt);
        uint64_t fv = 0, zb;
        memcpy(&zb, &z, 8);
        (void) hipMemcpy(&fv, fetch, 8, hipMemcpyDeviceToHost);
        ishmem_barrier_all();
        my_words();
        if (a != 0 || c != 0 || *(int *) hw.data() != 10 || (long) hw[1] != -2 || (long) fv != -3 || zb != 0x8000000000000000ull ||
            hw[2] != 0x8000000000000000ull)
            FAIL("[%d] FAIL host names: %d %ld word %d %ld fetch %ld double %llx: %s\n", pe, a, c, *(int *) hw.data(), (long) hw[1],
                 (long) fv, (unsigned long long) zb, ishmemi_c_last_error());
        ishmem_barrier_all();
    }

    ishmem_barrier_all();
    errors += ishmemi_c_error_count();
    (void) hipHostFree(bad);
    (void) hipFree(fetch);
    (void) hipFree(out);
    ishmem_free(gath);
    ishmem_free(w);
    ishmem_finalize();
    printf("[%d] %ld cases on %d PEs\n", pe, cases, npes);
    printf("%s errors %d\n", errors ? "FAIL" : "PASS", errors);
    return errors ? 1 : 0;
}
