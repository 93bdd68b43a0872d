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

// ---- strided / blocked put / get (ishmem_iput / iget, ishmemx_ibput / ibget) --------
// nblocks blocks of ipb items of W bytes; block b starts at src + b * src_stride and lands at
// dst + b * dst_stride.  W (1, 2, 4, 8 or 16) divides both bases, the block's byte length and both
// byte strides (runtime.cpp strided_plan), so every access is naturally aligned and misalignment only
// narrows the item.  The work is the nblocks * ipb items in block order: consecutive lanes take
// consecutive items of a block and then the next block's, so a block of 64 B or more is read and
// written in whole 64-B runs.
//
// Addressing: BOTH sides through per-lane 64-bit pointers (global loads / stores), not buffer
// descriptors.  A descriptor's offset is 32 bits wide and one wave's 64 items can sit 64 strides
// apart, so no re-based descriptor covers every stride; a lane's address here is
// base + b * stride + w * W evaluated in 64 bits, and the host has checked that the whole extent
// ((nblocks - 1) * stride + block bytes) neither overflows 64 bits nor leaves the buffer, so no
// term can wrap however far the extent passes 4 GiB.
//
// Cache policy as rma_copy_kernel: put = local loads nontemporal, remote stores write-through
// (sc0 sc1); get = remote loads sc0 sc1, local stores streaming.  All of them are vector memory
// instructions: nothing of a peer's is read through the scalar cache.
template <int W>
struct StridedItem;
template <>
struct StridedItem<1> {
    using type = uint8_t;
};
template <>
struct StridedItem<2> {
    using type = uint16_t;
};
template <>
struct StridedItem<4> {
    using type = uint32_t;
};
template <>
struct StridedItem<8> {
    using type = uint64_t;
};
template <>
struct StridedItem<16> {
    using type = u32x4;
};
typedef __attribute__((address_space(1))) u32x4 global_u32x4;

// System-coherent (sc0 sc1) access through a per-lane pointer.
template <typename I>
__device__ __forceinline__ I sys_ptr_load(const char *p)
{
    if constexpr (sizeof(I) == 16) return __builtin_amdgcn_global_load_b128((global_u32x4 *) p, "");
    else return __hip_atomic_load((const I *) p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <typename I>
__device__ __forceinline__ void sys_ptr_store(char *p, const I &v)
{
    if constexpr (sizeof(I) == 16) __builtin_amdgcn_global_store_b128((global_u32x4 *) p, v, "");
    else __hip_atomic_store((I *) p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ONE: ipb == 1 (every plain iput / iget whose elements are not wider than the item): item g is
// block g, no division.  Otherwise one 64-bit division per thread per tile finds the thread's first
// item's (block, item in block); its other kRmaUnroll - 1 items follow by stepping kRmaBlock items.
template <bool PUT, int W, bool ONE>
__global__ __launch_bounds__(kRmaBlock) void rma_strided_kernel(StridedArgs a)
{
    using I = typename StridedItem<W>::type;
    const uint32_t tid = threadIdx.x;
    const uint64_t nitems = a.nblocks * a.ipb;
    const uint64_t ntiles = (nitems + kRmaTile - 1) / kRmaTile;
    uint64_t step_b = 0, step_w = 0;  // kRmaBlock items further on = step_b blocks and step_w items
    if constexpr (!ONE) {
        step_b = (uint64_t) kRmaBlock / a.ipb;
        step_w = (uint64_t) kRmaBlock - step_b * a.ipb;
    }
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i0 = t * kRmaTile;
        const uint32_t lim = (uint32_t) min((uint64_t) kRmaTile, nitems - i0);
        uint64_t b = i0 + tid, w = 0;
        if constexpr (!ONE) {
            b = (i0 + tid) / a.ipb;
            w = (i0 + tid) - b * a.ipb;
        }
        I x[kRmaUnroll];
        char *dp[kRmaUnroll];
#pragma unroll
        for (int u = 0; u < kRmaUnroll; ++u) {
            const uint32_t e = (uint32_t) u * kRmaBlock + tid;
            // Lanes past the tile's end load item 0 again (and store nothing): no branch round a load,
            // so all kRmaUnroll loads are in flight before the first store.
            const char *sp = e < lim ? a.src + b * a.src_stride + w * W : a.src;
            dp[u] = a.dst + b * a.dst_stride + w * W;
            if constexpr (PUT) x[u] = __builtin_nontemporal_load((const I *) sp);
            else x[u] = sys_ptr_load<I>(sp);
            if constexpr (ONE) {
                b += kRmaBlock;
            } else {
                b += step_b;
                w += step_w;
                if (w >= a.ipb) {
                    w -= a.ipb;
                    ++b;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kRmaUnroll; ++u) {
            const uint32_t e = (uint32_t) u * kRmaBlock + tid;
            if (e >= lim) continue;
            if constexpr (PUT) sys_ptr_store<I>(dp[u], x[u]);
            else __builtin_nontemporal_store(x[u], (I *) dp[u]);
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

namespace {

template <bool PUT, int W>
void launch_strided_w(const StridedArgs &a, unsigned grid, hipStream_t s)
{
    if (a.ipb == 1) hipLaunchKernelGGL((rma_strided_kernel<PUT, W, true>), dim3(grid), dim3(kRmaBlock), 0, s, a);
    else hipLaunchKernelGGL((rma_strided_kernel<PUT, W, false>), dim3(grid), dim3(kRmaBlock), 0, s, a);
}

template <bool PUT>
hipError_t launch_strided_dir(const StridedArgs &a, unsigned grid, hipStream_t s)
{
    switch (a.item) {
        case 1: launch_strided_w<PUT, 1>(a, grid, s); break;
        case 2: launch_strided_w<PUT, 2>(a, grid, s); break;
        case 4: launch_strided_w<PUT, 4>(a, grid, s); break;
        case 8: launch_strided_w<PUT, 8>(a, grid, s); break;
        case 16: launch_strided_w<PUT, 16>(a, grid, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_rma_strided(const StridedArgs &a, bool put, int max_blocks, hipStream_t s)
{
    if (a.nblocks == 0 || a.ipb == 0) return hipSuccess;
    const uint64_t nitems = a.nblocks * a.ipb;
    const uint64_t ntiles = (nitems + kRmaTile - 1) / kRmaTile;
    const uint64_t cap = ISHMEMI_RMA_UNCAPPED ? (1ull << 31) - 1 : (uint64_t) std::max(1, max_blocks);
    const unsigned grid = (unsigned) std::max<uint64_t>(1, std::min<uint64_t>(ntiles, cap));
    return put ? launch_strided_dir<true>(a, grid, s) : launch_strided_dir<false>(a, grid, s);
}

}  // namespace ishmemi
