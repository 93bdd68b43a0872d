// ishmem_amd — put / get: one streaming peer-copy kernel behind the host blocking, _nbi and
// _on_stream forms (ishmem_put / ishmem_get and their kin, src/ishmem.h:90-330; the reference's
// intra-node path is a work-group copy to the peer's mapped heap, src/rma_impl.h:46-75, :116-145).
//
// One side of the copy is this PE's memory (heap, device or pinned host), the other a peer's heap
// mapped here.  The STORE side sets the layout: a head of < 16 bytes up to dest's first 16-B
// boundary, a body of 16-B items, a tail of < 16 bytes.  The load side is read at the same item
// offsets; when it sits on another 16-B phase those are unaligned 16-B loads (the hardware splits a
// load that crosses a line, as in the shifted reduce-scatter and the phased collect).
//   put: local loads nontemporal, remote stores system-coherent write-through (sc0 sc1): no line of
//        the peer's heap stays dirty in this XCD's L2, so the bytes are in memory when the kernel
//        completes and the target's next acquire (kernel start, or a device barrier) finds them.
//   get: remote loads system-coherent (sc0 sc1, never served from a stale L1 / L2 copy of bytes the
//        peer has since rewritten), local stores streaming.
// Every load goes through a buffer descriptor (vector memory path; nothing of a peer's is read
// through the scalar cache).  kUnroll items per thread per step are all issued before the first
// store; a grid-stride loop over tiles of kBlock * kUnroll items (16 KiB), the grid bounded by
// max_blocks.
#include "kernels_impl.h"

// A/B builds only (python -m ishmem_amd._build --define ...): another workgroup size, items per
// thread per step, or a grid of one workgroup per tile whatever max_blocks says.
#ifndef ISHMEMI_RMA_BLOCK
#define ISHMEMI_RMA_BLOCK kBlock
#endif
#ifndef ISHMEMI_RMA_UNROLL
#define ISHMEMI_RMA_UNROLL kUnroll
#endif
#ifndef ISHMEMI_RMA_UNCAPPED
#define ISHMEMI_RMA_UNCAPPED 0
#endif

namespace ishmemi {
namespace {

constexpr int kRmaBlock = ISHMEMI_RMA_BLOCK, kRmaUnroll = ISHMEMI_RMA_UNROLL;
constexpr uint64_t kRmaTile = (uint64_t) kRmaBlock * kRmaUnroll;  // items per tile

template <bool PUT>
__global__ __launch_bounds__(kRmaBlock) void rma_copy_kernel(RmaArgs a)
{
    constexpr int kLoad = PUT ? kNonTemporal : kSysCoherent;
    const uint32_t tid = threadIdx.x;
    const char *sb = a.src + a.head;
    char *db = a.dst + a.head;
    const uint64_t ntiles = (a.nitems + kRmaTile - 1) / kRmaTile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i0 = t * kRmaTile;
        const uint32_t lim = (uint32_t) min((uint64_t) kRmaTile, a.nitems - i0);
        // Descriptors based at the tile (offsets < 16 KiB, any payload size).
        const __amdgpu_buffer_rsrc_t lr = make_rsrc(uniform_ptr(sb + i0 * 16));
        u32x4 x[kRmaUnroll];
#pragma unroll
        for (int u = 0; u < kRmaUnroll; ++u) {
            const uint32_t e = (uint32_t) u * kRmaBlock + tid;
            if (e < lim) x[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(lr, e * 16u, 0, kLoad));
        }
        if constexpr (PUT) {
            const __amdgpu_buffer_rsrc_t dr = make_rsrc(uniform_ptr(db + i0 * 16));
#pragma unroll
            for (int u = 0; u < kRmaUnroll; ++u) {
                const uint32_t e = (uint32_t) u * kRmaBlock + tid;
                if (e < lim) wt_store(dr, e * 16u, x[u]);
            }
        } else {
            u32x4 *dp = (u32x4 *) (db + i0 * 16);
#pragma unroll
            for (int u = 0; u < kRmaUnroll; ++u) {
                const uint32_t e = (uint32_t) u * kRmaBlock + tid;
                if (e < lim) nt_store(dp + e, x[u]);
            }
        }
    }
    // Head and tail bytes (< 16 each) by the first workgroup; descriptors based at the region.
    if (blockIdx.x == 0 && tid < 16) {
        for (int region = 0; region < 2; ++region) {
            const uint64_t cnt = region == 0 ? a.head : a.tail;
            const uint64_t rbase = region == 0 ? 0 : a.head + a.nitems * 16;
            if (tid >= cnt) continue;
            const uint8_t b = cload<uint8_t>(make_rsrc(a.src + rbase), tid);
            if constexpr (PUT) wt_store(make_rsrc(a.dst + rbase), tid, b);
            else a.dst[rbase + tid] = (char) b;
        }
    }
}

// Test hook (ishmemi_c_read_all_u32): EVERY workgroup reads all n words of p with ordinary loads and
// writes its own copy, out[b * n + i] = p[i] — what a user's consumer kernel does.  Run before a
// peer's put it leaves p's lines in the L1 of every CU it ran on and in those XCDs' L2s; run after,
// it shows what plain loads then see.
__global__ __launch_bounds__(256) void read_all_u32_kernel(uint32_t *out, const uint32_t *p, uint64_t n)
{
    uint32_t *mine = out + (uint64_t) blockIdx.x * n;
    for (uint64_t i = threadIdx.x; i < n; i += 256) mine[i] = p[i];
}

}  // namespace

hipError_t launch_read_all_u32(uint32_t *out, const uint32_t *p, uint64_t n, int grid, hipStream_t s)
{
    if (n == 0 || grid < 1) return hipSuccess;
    hipLaunchKernelGGL(read_all_u32_kernel, dim3((unsigned) grid), dim3(256), 0, s, out, p, n);
    return hipGetLastError();
}

hipError_t launch_rma_copy(const RmaArgs &a, bool put, int max_blocks, hipStream_t s)
{
    const uint64_t ntiles = (a.nitems + kRmaTile - 1) / kRmaTile;
    const uint64_t cap = ISHMEMI_RMA_UNCAPPED ? (1ull << 31) - 1 : (uint64_t) std::max(1, max_blocks);
    const unsigned grid = (unsigned) std::max<uint64_t>(1, std::min<uint64_t>(ntiles, cap));
    if (put) hipLaunchKernelGGL(rma_copy_kernel<true>, dim3(grid), dim3(kRmaBlock), 0, s, a);
    else hipLaunchKernelGGL(rma_copy_kernel<false>, dim3(grid), dim3(kRmaBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace ishmemi
