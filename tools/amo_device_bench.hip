// Device-initiated fetching atomics per microsecond on a peer's word (dev tool, run by
// tools/amo_sweep.py with 2 co-located PEs).  PE 0's kernel: every lane does kOps
// ishmem_uint64_atomic_fetch_add(word, 1, 1) — on ONE word of PE 1 ("one"), or on one word per wave,
// 64 B apart ("per_wave") — for 1 wave, 1 workgroup, 64 and 256 workgroups of 256 threads; timed with
// HIP events, kRounds windows per shape after a warm-up.  PE 1 waits on the host.  The count is of
// lane operations: for a wave-uniform address the compiler folds a wave's adds into one hardware
// atomic, so the hardware sees 1/64 of them.  Prints CSV rows: shape,words,lanes,ops,us...
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include <ishmem.h>

constexpr int kOps = 64, kRounds = 9;

__global__ void bench_kernel(uint64_t *words, int per_wave, int pe, uint64_t *sink)
{
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t *w = words + (per_wave ? (size_t) (gid / 64) * 8 : 0);
    uint64_t acc = 0;
    for (int i = 0; i < kOps; ++i) acc += ishmem_uint64_atomic_fetch_add(w, (uint64_t) 1, pe);
    if (acc == 1) sink[0] = acc;  // keeps the fetched values alive
}

int main()
{
    ishmem_init();
    const int pe = ishmem_my_pe(), npes = ishmem_n_pes();
    const int peer = npes > 1 ? 1 : 0;
    constexpr int kMaxWaves = 256 * 4;
    uint64_t *words = (uint64_t *) ishmem_calloc((size_t) kMaxWaves * 8 + 8, 8);
    uint64_t *sink = words + (size_t) kMaxWaves * 8;
    hipEvent_t e0, e1;
    (void) hipEventCreate(&e0);
    (void) hipEventCreate(&e1);
    ishmem_barrier_all();
    if (pe == 0) {
        const struct { const char *name; int grid, block; } shapes[] = {
            {"1_wave", 1, 64}, {"1_workgroup", 1, 256}, {"64_workgroups", 64, 256}, {"256_workgroups", 256, 256}};
        for (const auto &s : shapes)
            for (int per_wave = 0; per_wave < 2; ++per_wave) {
                std::vector<float> us;
                for (int r = 0; r < kRounds + 1; ++r) {
                    (void) hipEventRecord(e0, 0);
                    hipLaunchKernelGGL(bench_kernel, dim3(s.grid), dim3(s.block), 0, 0, words, per_wave, peer, sink);
                    (void) hipEventRecord(e1, 0);
                    if (hipEventSynchronize(e1) != hipSuccess) return 1;
                    float ms = 0;
                    (void) hipEventElapsedTime(&ms, e0, e1);
                    if (r) us.push_back(ms * 1000.0f);  // the first window warms up
                }
                std::sort(us.begin(), us.end());
                const double ops = (double) s.grid * s.block * kOps;
                printf("AMODEV,%s,%s,%d,%.0f,%.2f,%.2f,%.2f,%.1f\n", s.name, per_wave ? "per_wave" : "one", s.grid * s.block, ops,
                       us[kRounds / 2], us[kRounds / 4], us[3 * kRounds / 4], ops / us[kRounds / 2]);
            }
    }
    ishmem_barrier_all();
    ishmem_free(words);
    ishmem_finalize();
    return 0;
}
