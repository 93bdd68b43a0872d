// Device-initiated collectives (include/ishmemx_device.h) on wide and strided teams, at byte
// offsets, with guard bytes round every dest: the cases tests/cpp/device_wg.hip does not reach.
//   teams     WORLD plus strided / offset / one-member splits (table in main); widths up to 8, so
//             the member-batch fold of reduce_group runs a second, a partial and a carried batch;
//             a PE's team index differs from its PE number; non-members pass ISHMEM_TEAM_INVALID
//   buffers   dest sits in a block filled with 0xA5, >= 64 guard bytes on each side, and the whole
//             block is compared after every case; dest / source at byte offsets
//             {0, sizeof(T), 16 - sizeof(T)}^2, so the element-wise arms run as the whole body
//   checker   oracle_reduce_fold / oracle_combine over seeded oracle_fill_random inputs in team
//             order, bit-exact for every type; closed-form bytes for collect / broadcast / alltoall
//   special   NaN, infinities, signed zeros, overflow and subnormals (oracle_fill_special) through
//             the FP reduces and sum scans, compared by special_rule(): NaN where the team-order
//             fold is NaN, a zero of either sign for max / min over zeros of both signs, the
//             oracle's bits everywhere else
// A device collective that returns non-zero on a member (a barrier timed out) leaves the members
// out of step: the program prints the FAIL line and stops there.
// Launch: ISHMEM_PE=<pe> ISHMEM_NPES=<n> ISHMEM_DEVICE=0 ISHMEM_BOOTSTRAP_KEY=<k> ./device_teams
#include <hip/hip_cooperative_groups.h>
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "ishmem.h"
#include "ishmemx.h"

namespace cg = cooperative_groups;

extern "C" {
#include "oracle.h"
}

struct Team {
    int h;  // this PE's handle (ISHMEM_TEAM_INVALID on a non-member)
    int start, stride, size;
    int me;  // this PE's index in the team, -1 on a non-member
};

static int errors = 0, g_pe = -1;
static char *sb = nullptr, *db = nullptr;  // symmetric source / dest blocks
static int *rc = nullptr;                  // answers of the query kernel, 32 ints
static std::vector<unsigned char> hostblk;
constexpr size_t kBlk = 128 << 10;
constexpr size_t kGuard = 64;
static const char *const kOpName[7] = {"and", "or", "xor", "max", "min", "sum", "prod"};
static const char *const kGrpName[3] = {"block", "tile", "item"};

template <typename T>
struct TI;
#define TYPE_INFO(T, ODT, NAME)                     \
    template <>                                     \
    struct TI<T> {                                  \
        static constexpr int odt = ODT;             \
        static constexpr const char *name = NAME;   \
    };
TYPE_INFO(int8_t, OD_INT8, "int8")
TYPE_INFO(uint8_t, OD_UINT8, "uint8")
TYPE_INFO(uint16_t, OD_UINT16, "uint16")
TYPE_INFO(int32_t, OD_INT32, "int32")
TYPE_INFO(long, OD_INT64, "long")
TYPE_INFO(uint64_t, OD_UINT64, "uint64")
TYPE_INFO(float, OD_FLOAT, "float")
TYPE_INFO(double, OD_DOUBLE, "double")
#undef TYPE_INFO

// ---- kernels --------------------------------------------------------------------------------
template <int OPC, typename T, typename G>
__device__ int reduce_by_group(int team, T *d, const T *s, size_t n, const G &g)
{
    if constexpr (OPC == ISHMEMI_OP_AND) return ishmemx_and_reduce_work_group(team, d, s, n, g);
    else if constexpr (OPC == ISHMEMI_OP_OR) return ishmemx_or_reduce_work_group(team, d, s, n, g);
    else if constexpr (OPC == ISHMEMI_OP_XOR) return ishmemx_xor_reduce_work_group(team, d, s, n, g);
    else if constexpr (OPC == ISHMEMI_OP_MAX) return ishmemx_max_reduce_work_group(team, d, s, n, g);
    else if constexpr (OPC == ISHMEMI_OP_MIN) return ishmemx_min_reduce_work_group(team, d, s, n, g);
    else if constexpr (OPC == ISHMEMI_OP_SUM) return ishmemx_sum_reduce_work_group(team, d, s, n, g);
    else return ishmemx_prod_reduce_work_group(team, d, s, n, g);
}

template <int OPC, typename T>
__device__ int reduce_by_item(int team, T *d, const T *s, size_t n)
{
    if constexpr (OPC == ISHMEMI_OP_AND) return ishmem_and_reduce(team, d, s, n);
    else if constexpr (OPC == ISHMEMI_OP_OR) return ishmem_or_reduce(team, d, s, n);
    else if constexpr (OPC == ISHMEMI_OP_XOR) return ishmem_xor_reduce(team, d, s, n);
    else if constexpr (OPC == ISHMEMI_OP_MAX) return ishmem_max_reduce(team, d, s, n);
    else if constexpr (OPC == ISHMEMI_OP_MIN) return ishmem_min_reduce(team, d, s, n);
    else if constexpr (OPC == ISHMEMI_OP_SUM) return ishmem_sum_reduce(team, d, s, n);
    else return ishmem_prod_reduce(team, d, s, n);
}

// mode 0: the whole thread block; 1: a 64-lane tile (the block's second wavefront, the other
// waves return); 2: one work-item.
template <typename T, int OPC>
__global__ void reduce_kernel(int team, T *dest, const T *source, size_t n, int mode, int *rc)
{
    auto blk = cg::this_thread_block();
    if (mode == 0) {
        const int r = reduce_by_group<OPC>(team, dest, source, n, blk);
        if (threadIdx.x == 0) *rc = r;
    } else if (mode == 1) {
        auto tile = cg::tiled_partition<64>(blk);
        if (threadIdx.x / warpSize != 1) return;
        const int r = reduce_by_group<OPC>(team, dest, source, n, tile);
        if (__lane_id() == 0) *rc = r;
    } else {
        if (threadIdx.x != 0) return;
        *rc = reduce_by_item<OPC>(team, dest, source, n);
    }
}

template <typename T>
__device__ int inscan_by_item(int team, T *d, const T *s, size_t n)
{
    if constexpr (std::is_same_v<T, float>) return ishmem_float_sum_inscan(team, d, s, n);
    else if constexpr (std::is_same_v<T, double>) return ishmem_double_sum_inscan(team, d, s, n);
    else if constexpr (std::is_same_v<T, int8_t>) return ishmem_int8_sum_inscan(team, d, s, n);
    else if constexpr (std::is_same_v<T, uint16_t>) return ishmem_uint16_sum_inscan(team, d, s, n);
    else if constexpr (std::is_same_v<T, int32_t>) return ishmem_int32_sum_inscan(team, d, s, n);
    else return ishmem_uint64_sum_inscan(team, d, s, n);
}

template <typename T>
__global__ void scan_kernel(int team, T *dest, const T *source, size_t n, int mode, int incl, int *rc)
{
    auto blk = cg::this_thread_block();
    if (mode == 0) {
        const int r = incl ? ishmemx_sum_inscan_work_group(team, dest, source, n, blk)
                           : ishmemx_sum_exscan_work_group(team, dest, source, n, blk);
        if (threadIdx.x == 0) *rc = r;
    } else if (mode == 1) {
        auto tile = cg::tiled_partition<64>(blk);
        if (threadIdx.x / warpSize != 1) return;
        const int r = incl ? ishmemx_sum_inscan_work_group(team, dest, source, n, tile)
                           : ishmemx_sum_exscan_work_group(team, dest, source, n, tile);
        if (__lane_id() == 0) *rc = r;
    } else {
        if (threadIdx.x != 0) return;
        *rc = inscan_by_item<T>(team, dest, source, n);
    }
}

enum { F_COLLECT = 0, F_FCOLLECT, F_COLLECTMEM, F_FCOLLECTMEM, F_BROADCAST, F_BROADCASTMEM, F_ALLTOALL, F_COUNT };
static const char *const kFormName[F_COUNT] = {"collect",   "fcollect",     "collectmem", "fcollectmem",
                                               "broadcast", "broadcastmem", "alltoall"};

template <typename T>
__global__ void coll_kernel(int form, int team, T *dest, const T *source, size_t n, int root, int *rc)
{
    auto blk = cg::this_thread_block();
    int r;
    if (form == F_COLLECT) r = ishmemx_collect_work_group(team, dest, source, n, blk);
    else if (form == F_FCOLLECT) r = ishmemx_fcollect_work_group(team, dest, source, n, blk);
    else if (form == F_COLLECTMEM) r = ishmemx_collectmem_work_group(team, dest, source, n * sizeof(T), blk);
    else if (form == F_FCOLLECTMEM) r = ishmemx_fcollectmem_work_group(team, dest, source, n * sizeof(T), blk);
    else if (form == F_BROADCAST) r = ishmemx_broadcast_work_group(team, dest, source, n, root, blk);
    else if (form == F_BROADCASTMEM) r = ishmemx_broadcastmem_work_group(team, dest, source, n * sizeof(T), root, blk);
    else r = ishmemx_alltoall_work_group(team, dest, source, n, blk);
    if (threadIdx.x == 0) *rc = r;
}

__global__ void query_kernel(int team, int size, int *out)
{
    out[0] = ishmem_team_my_pe(team);
    out[1] = ishmem_team_n_pes(team);
    for (int i = 0; i <= size; ++i) out[2 + i] = ishmem_team_translate_pe(team, i, ISHMEM_TEAM_WORLD);
}

// ---- host side --------------------------------------------------------------------------------
static void fail(const char *form, int mode, int block, const Team &t, const char *type, const char *op, size_t n,
                 int d, int s, int r, size_t bad)
{
    if (++errors <= 16)
        printf("[%d] FAIL %s group %s block %d team (%d,%d,%d) type %s op %s n %zu doff %d soff %d rc %d bad-bytes %zu\n",
               g_pe, form, kGrpName[mode], block, t.start, t.stride, t.size, type, op, n, d, s, r, bad);
}

[[noreturn]] static void stop(const char *why)
{
    ++errors;
    printf("[%d] FAIL stopping: %s\n[%d] FAIL errors %d\n", g_pe, why, g_pe, errors);
    fflush(stdout);
    _exit(1);
}

static uint64_t mix(uint64_t h, uint64_t v)
{
    h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
    return h * 0xD6E8FEB86659FD93ull;
}

// One seed per (case, member); every member of the team derives the same ones.
static uint64_t case_seed(int tag, int ti, int odt, int op, size_t n, int mode, int block, int d, int s, int j)
{
    uint64_t h = 0x15AE0007ull;
    for (uint64_t v : {(uint64_t) tag, (uint64_t) ti, (uint64_t) odt, (uint64_t) op, (uint64_t) n, (uint64_t) mode,
                       (uint64_t) block, (uint64_t) d, (uint64_t) s, (uint64_t) j})
        h = mix(h, v);
    return h | 1;
}

// Block length for a payload of nb bytes at offset kGuard + d (d < 16): guards on both sides
// and an unused rest.  The kernel's return code lands in the word right after the block, so one
// copy fetches both.
static size_t block_len(size_t nb)
{
    const size_t len = ((kGuard + 16 + nb + kGuard + 63) & ~(size_t) 63) + 64;
    if (len + 64 > kBlk) stop("case larger than the test block");
    return len;
}

static int *rc_of(size_t len) { return (int *) (db + len); }
constexpr int kRcUnset = (int) 0xA5A5A5A5;  // what fill_block leaves there

static void fill_block(size_t len) { (void) hipMemset(db, 0xA5, len + 64); }  // rc reads non-zero until written

// Waits for the kernel and fetches the dest block and rc.  Any HIP error ends the program.
static int finish(size_t len)
{
    const hipError_t e = hipMemcpy(hostblk.data(), db, len + 64, hipMemcpyDeviceToHost);
    if (e != hipSuccess) stop(hipGetErrorString(e));
    int r;
    memcpy(&r, hostblk.data() + len, sizeof(int));
    return r;
}

// Bytes of the block that differ from: `want` at [off, off + nb), 0xA5 everywhere else.
static size_t check_block(size_t len, size_t off, const void *want, size_t nb)
{
    const unsigned char *w = (const unsigned char *) want;
    size_t bad = 0;
    for (size_t i = 0; i < len; ++i) bad += hostblk[i] != ((i >= off && i < off + nb) ? w[i - off] : 0xA5);
    return bad;
}

static std::vector<std::pair<int, int>> offset_pairs(int sz)
{
    const int a = sz, b = 16 - sz;
    // aligned; same non-zero phase; different phases; (0, s != 0); (d != 0, 0)
    const std::pair<int, int> cand[5] = {{0, 0}, {a, a}, {a, b}, {0, a}, {b, 0}};
    std::vector<std::pair<int, int>> out;
    for (const auto &p : cand)
        if (std::find(out.begin(), out.end(), p) == out.end()) out.push_back(p);
    return out;
}

static std::vector<size_t> unique_sizes(std::vector<size_t> v)
{
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    v.erase(std::remove(v.begin(), v.end(), (size_t) 0), v.end());
    return v;
}

// The reduce-scatter chunk is per = roundup64(ceil(n / size)); a 64-thread group steps 64 * 4 items
// of E elements.
static std::vector<size_t> reduce_sizes(int size, size_t E)
{
    const size_t p = (size_t) size, per = 2 * 64 * 4 * E + 64;
    return unique_sizes({1, p - 1, 64 * p - 1, 64 * p + 1, 64 * (p - 1) + E + 1, p * per - (64 - E - 1)});
}

template <typename T, int OPC>
static void reduce_case(const Team &t, int ti, int mode, int block, size_t n, int d, int s, bool inplace)
{
    constexpr int ODT = TI<T>::odt;
    constexpr bool prod_fp = (ODT >= OD_FLOAT) && OPC == OR_PROD;
    std::vector<std::vector<T>> src((size_t) t.size, std::vector<T>(n));
    std::vector<const void *> ptrs((size_t) t.size);
    for (int j = 0; j < t.size; ++j) {
        oracle_fill_random(ODT, case_seed(inplace ? 2 : 1, ti, ODT, OPC, n, mode, block, d, s, j), prod_fp ? 0.5 : -1.0,
                           prod_fp ? 2.0 : 1.0, n, src[(size_t) j].data());
        ptrs[(size_t) j] = src[(size_t) j].data();
    }
    std::vector<T> want(n);
    oracle_reduce_fold(OPC, ODT, ptrs.data(), t.size, 0, want.data(), n);
    const size_t nb = n * sizeof(T), len = block_len(nb);
    fill_block(len);
    T *dst = (T *) (db + kGuard + d);
    const T *sp = inplace ? (const T *) dst : (const T *) (sb + kGuard + s);
    (void) hipMemcpy((void *) sp, src[(size_t) t.me].data(), nb, hipMemcpyHostToDevice);
    hipLaunchKernelGGL((reduce_kernel<T, OPC>), dim3(1), dim3(mode == 0 ? block : mode == 1 ? 256 : 1), 0, 0, t.h, dst,
                       sp, n, mode, rc_of(len));
    const int r = finish(len);
    const size_t bad = check_block(len, kGuard + d, want.data(), nb);
    if (r != 0 || bad) fail(inplace ? "reduce-in-place" : "reduce", mode, block, t, TI<T>::name, kOpName[OPC], n, d, s, r, bad);
    if (r != 0) stop("a device reduce returned non-zero on a member");
}

// The special-value comparison rule (DESIGN.md "Special values"), written once: `got` against the
// team-order fold `want` of the members `src[0 .. nsrc)`.  An element that is NaN in the fold must be
// NaN (any payload, any sign); a max / min that is zero while the column's non-NaN zeros carry both
// signs may be a zero of either sign (glibc and the GPU may differ); every other element must have
// the fold's bits.  A team of one copies: bits throughout.  Elements that meet a soft rule are
// copied into `want`, so check_block then compares the whole block, guards included.  Returns the
// number of elements that took a soft rule above the caps tests/special_values.py sets (a quarter
// NaN, a tenth either-zero), which the table never reaches: 0 for a sound case.
template <typename T>
static size_t special_rule(int op, const std::vector<std::vector<T>> &src, size_t nsrc, std::vector<T> &want,
                           const unsigned char *got_bytes)
{
    const size_t n = want.size();
    size_t nan = 0, zero = 0;
    for (size_t i = 0; i < n; ++i) {
        T got;
        memcpy(&got, got_bytes + i * sizeof(T), sizeof(T));
        if (nsrc < 2) continue;
        if (std::isnan(want[i])) {
            ++nan;
            if (std::isnan(got)) want[i] = got;
            continue;
        }
        if ((op == OR_MAX || op == OR_MIN) && want[i] == 0) {
            bool pos = false, neg = false;
            for (size_t j = 0; j < nsrc; ++j)
                if (src[j][i] == 0) (std::signbit(src[j][i]) ? neg : pos) = true;
            if (pos && neg) {
                ++zero;
                if (got == 0) want[i] = got;
            }
        }
    }
    return (4 * nan > n ? nan : 0) + (10 * zero > n ? zero : 0);
}

// A reduce over the special-value table: member j's source from oracle_fill_special, the expected
// values from oracle_reduce_fold, compared by special_rule.
template <typename T, int OPC>
static void reduce_special_case(const Team &t, int ti, int mode, int block, size_t n, int d, int s)
{
    constexpr int ODT = TI<T>::odt;
    std::vector<std::vector<T>> src((size_t) t.size, std::vector<T>(n));
    std::vector<const void *> ptrs((size_t) t.size);
    for (int j = 0; j < t.size; ++j) {
        if (oracle_fill_special(ODT, j, t.size, n, src[(size_t) j].data())) stop("oracle_fill_special failed");
        ptrs[(size_t) j] = src[(size_t) j].data();
    }
    std::vector<T> want(n);
    oracle_reduce_fold(OPC, ODT, ptrs.data(), t.size, 0, want.data(), n);
    const size_t nb = n * sizeof(T), len = block_len(nb);
    fill_block(len);
    T *dst = (T *) (db + kGuard + d);
    const T *sp = (const T *) (sb + kGuard + s);
    (void) hipMemcpy((void *) sp, src[(size_t) t.me].data(), nb, hipMemcpyHostToDevice);
    hipLaunchKernelGGL((reduce_kernel<T, OPC>), dim3(1), dim3(mode == 0 ? block : mode == 1 ? 256 : 1), 0, 0, t.h, dst,
                       sp, n, mode, rc_of(len));
    const int r = finish(len);
    const size_t capped = special_rule<T>(OPC, src, (size_t) t.size, want, hostblk.data() + kGuard + d);
    const size_t bad = check_block(len, kGuard + d, want.data(), nb) + capped;
    if (r != 0 || bad) fail("reduce-special", mode, block, t, TI<T>::name, kOpName[OPC], n, d, s, r, bad);
    if (r != 0) stop("a device reduce returned non-zero on a member");
}

// max / min / sum / prod over the table in the block, tile and one-work-item modes, at n = E + 1 and
// 2 * 64 * 4 * E + E + 1, aligned and with dest and source on different phases.
template <typename T>
static void reduce_special_sweep(const Team &t, int ti)
{
    const size_t E = 16 / sizeof(T);
    const int a = (int) sizeof(T), b = 16 - (int) sizeof(T);
    for (size_t n : {E + 1, 2 * 64 * 4 * E + E + 1})
        for (const auto &p : {std::pair<int, int>{0, 0}, std::pair<int, int>{a, b}})
            for (int mode = 0; mode < 3; ++mode) {
                const int block = mode == 0 ? (n > E + 1 ? 256 : 64) : mode == 1 ? 256 : 1;
                reduce_special_case<T, OR_MAX>(t, ti, mode, block, n, p.first, p.second);
                reduce_special_case<T, OR_MIN>(t, ti, mode, block, n, p.first, p.second);
                reduce_special_case<T, OR_SUM>(t, ti, mode, block, n, p.first, p.second);
                reduce_special_case<T, OR_PROD>(t, ti, mode, block, n, p.first, p.second);
            }
}

// One reduce case with the op chosen at run time (FP types have max, min, sum and prod only).
template <typename T>
static void reduce_op_case(int op, const Team &t, int ti, int mode, int block, size_t n, int d, int s, bool inplace)
{
    if constexpr (!std::is_floating_point_v<T>) {
        if (op == OR_AND) return reduce_case<T, OR_AND>(t, ti, mode, block, n, d, s, inplace);
        if (op == OR_OR) return reduce_case<T, OR_OR>(t, ti, mode, block, n, d, s, inplace);
        if (op == OR_XOR) return reduce_case<T, OR_XOR>(t, ti, mode, block, n, d, s, inplace);
    }
    if (op == OR_MAX) return reduce_case<T, OR_MAX>(t, ti, mode, block, n, d, s, inplace);
    if (op == OR_MIN) return reduce_case<T, OR_MIN>(t, ti, mode, block, n, d, s, inplace);
    if (op == OR_SUM) return reduce_case<T, OR_SUM>(t, ti, mode, block, n, d, s, inplace);
    if (op == OR_PROD) return reduce_case<T, OR_PROD>(t, ti, mode, block, n, d, s, inplace);
    stop("op not valid for the type");
}

// For one type: every n x every offset pair x every group (the geometry decides which loops, arms
// and chunk edges of reduce_group run).  The op only changes the element function, so it is not
// crossed with the geometry but taken in turn, op = (n index + pair index + group index + team
// index) mod the number of ops: every op of the type then meets every offset pair (the aligned
// one included), every group and a spread of n, on every team.
template <typename T>
static void reduce_sweep(const Team &t, int ti)
{
    constexpr bool fp = std::is_floating_point_v<T>;
    constexpr int first = fp ? OR_MAX : OR_AND, nops = fp ? 4 : 7;
    const auto ns = reduce_sizes(t.size, 16 / sizeof(T));
    const auto pairs = offset_pairs((int) sizeof(T));
    for (size_t ni = 0; ni < ns.size(); ++ni)
        for (size_t pi = 0; pi < pairs.size(); ++pi) {
            const int k = (int) (ni + pi) + ti, d = pairs[pi].first, s = pairs[pi].second;
            reduce_op_case<T>(first + k % nops, t, ti, 0, 64, ns[ni], d, s, false);
            reduce_op_case<T>(first + (k + 1) % nops, t, ti, 0, 256, ns[ni], d, s, false);
            reduce_op_case<T>(first + (k + 2) % nops, t, ti, 1, 256, ns[ni], d, s, false);
        }
    // One work-item: the two smallest n, consecutive ops (eight or ten cases: every op runs).
    for (size_t i = 0; i < 2 && i < ns.size(); ++i)
        for (size_t pi = 0; pi < pairs.size(); ++pi)
            reduce_op_case<T>(first + (int) (i * pairs.size() + pi) % nops, t, ti, 2, 1, ns[i], pairs[pi].first,
                              pairs[pi].second, false);
}

// In place (dest == source), aligned and on a non-zero phase, every n and group.
template <typename T, int OPC>
static void reduce_inplace_sweep(const Team &t, int ti)
{
    for (size_t n : reduce_sizes(t.size, 16 / sizeof(T)))
        for (int d : {0, (int) sizeof(T)}) {
            reduce_case<T, OPC>(t, ti, 0, 64, n, d, d, true);
            reduce_case<T, OPC>(t, ti, 0, 256, n, d, d, true);
            reduce_case<T, OPC>(t, ti, 1, 256, n, d, d, true);
        }
}

static void reduce_suite(const Team &t, int ti)
{
    reduce_sweep<int8_t>(t, ti);
    reduce_sweep<uint16_t>(t, ti);
    reduce_sweep<int32_t>(t, ti);
    reduce_sweep<uint64_t>(t, ti);
    reduce_sweep<float>(t, ti);
    reduce_sweep<double>(t, ti);
    // In place for one type per op.
    reduce_inplace_sweep<int8_t, OR_AND>(t, ti);
    reduce_inplace_sweep<uint16_t, OR_OR>(t, ti);
    reduce_inplace_sweep<int32_t, OR_XOR>(t, ti);
    reduce_inplace_sweep<uint64_t, OR_MAX>(t, ti);
    reduce_inplace_sweep<float, OR_MIN>(t, ti);
    reduce_inplace_sweep<double, OR_SUM>(t, ti);
    reduce_inplace_sweep<int32_t, OR_PROD>(t, ti);
    // NaN, infinities, signed zeros, overflow and subnormals.
    reduce_special_sweep<float>(t, ti);
    reduce_special_sweep<double>(t, ti);
}

// Prefix sums: a plain left-to-right fold in T over members 0..me (inclusive) or 0..me-1
// (exclusive; member 0 gets zeros).  The first term passes through unchanged: member 0's first
// FP element is -0.0 and must come back as -0.0.  special (FP types): member j's source from
// oracle_fill_special instead, the result compared by special_rule.
template <typename T>
static void scan_case(const Team &t, int ti, int mode, int block, size_t n, int d, int s, bool incl, bool special = false)
{
    constexpr int ODT = TI<T>::odt;
    std::vector<std::vector<T>> src((size_t) t.size, std::vector<T>(n));
    for (int j = 0; j < t.size; ++j) {
        if (special) {
            if (oracle_fill_special(ODT, j, t.size, n, src[(size_t) j].data())) stop("oracle_fill_special failed");
        } else {
            oracle_fill_random(ODT, case_seed(3, ti, ODT, incl, n, mode, block, d, s, j), -1.0, 1.0, n, src[(size_t) j].data());
        }
    }
    if constexpr (ODT >= OD_FLOAT)
        if (!special) src[0][0] = (T) -0.0;
    const int last = incl ? t.me : t.me - 1;
    std::vector<T> want(n, T());
    if (last >= 0) {
        want = src[0];
        for (int k = 1; k <= last; ++k) oracle_combine(OR_SUM, ODT, want.data(), src[(size_t) k].data(), n);
    }
    const size_t nb = n * sizeof(T), len = block_len(nb);
    fill_block(len);
    T *dst = (T *) (db + kGuard + d);
    const T *sp = (const T *) (sb + kGuard + s);
    (void) hipMemcpy((void *) sp, src[(size_t) t.me].data(), nb, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(scan_kernel<T>, dim3(1), dim3(mode == 0 ? block : mode == 1 ? 256 : 1), 0, 0, t.h, dst, sp, n,
                       mode, (int) incl, rc_of(len));
    const int r = finish(len);
    size_t capped = 0;
    if constexpr (ODT >= OD_FLOAT)
        if (special && last >= 1) capped = special_rule<T>(OR_SUM, src, (size_t) last + 1, want, hostblk.data() + kGuard + d);
    const size_t bad = check_block(len, kGuard + d, want.data(), nb) + capped;
    if (r != 0 || bad)
        fail(special ? (incl ? "sum_inscan-special" : "sum_exscan-special") : incl ? "sum_inscan" : "sum_exscan", mode, block, t,
             TI<T>::name, "sum", n, d, s, r, bad);
    if (r != 0) stop("a device scan returned non-zero on a member");
}

template <typename T>
static void scan_sweep(const Team &t, int ti)
{
    const size_t E = 16 / sizeof(T);
    const auto ns = unique_sizes({1, E - 1, E + 1, 2 * 64 * 4 * E + E + 1});
    const auto pairs = offset_pairs((int) sizeof(T));
    for (size_t n : ns)
        for (const auto &p : pairs) {
            for (bool incl : {true, false}) {
                scan_case<T>(t, ti, 0, 64, n, p.first, p.second, incl);
                scan_case<T>(t, ti, 0, 256, n, p.first, p.second, incl);
                scan_case<T>(t, ti, 1, 256, n, p.first, p.second, incl);
            }
            scan_case<T>(t, ti, 2, 1, n, p.first, p.second, true);  // ishmem_<T>_sum_inscan by one work-item
            if constexpr (std::is_floating_point_v<T>) {  // the special-value table, every group
                for (bool incl : {true, false}) {
                    scan_case<T>(t, ti, 0, n > E + 1 ? 256 : 64, n, p.first, p.second, incl, true);
                    scan_case<T>(t, ti, 1, 256, n, p.first, p.second, incl, true);
                }
                scan_case<T>(t, ti, 2, 1, n, p.first, p.second, true, true);
            }
        }
}

// dest overlapping source on a team of two or more: every member gets non-zero at once, and the
// block (source bytes inside, 0xA5 round them) stays as it was.
static void scan_overlap_case(const Team &t, int ti)
{
    if (t.size < 2) return;
    const size_t n = 5, nb = n * sizeof(int32_t), len = block_len(nb + sizeof(int32_t));
    std::vector<int32_t> src(n);
    for (bool incl : {true, false}) {
        oracle_fill_random(OD_INT32, case_seed(4, ti, OD_INT32, incl, n, 0, 64, 4, 0, t.me), 0, 0, n, src.data());
        fill_block(len);
        int32_t *sp = (int32_t *) (db + kGuard), *dst = sp + 1;
        (void) hipMemcpy(sp, src.data(), nb, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(scan_kernel<int32_t>, dim3(1), dim3(64), 0, 0, t.h, dst, (const int32_t *) sp, n, 0, (int) incl, rc_of(len));
        const int r = finish(len);
        const size_t bad = check_block(len, kGuard, src.data(), nb);
        if (r == 0 || r == kRcUnset || bad) fail(incl ? "sum_inscan-overlap" : "sum_exscan-overlap", 0, 64, t, "int32", "sum", n, 4, 0, r, bad);
    }
}

// collect / fcollect / broadcast / alltoall, typed and mem forms.  Byte b of member j's source is
// pat(j, b), a closed form of b, the member's PE number, the team, n and the form.  collect:
// member j contributes (j % 3 == 1) ? 0 : n + 5 j elements.
template <typename T>
static void coll_case(const Team &t, int ti, int form, int block, size_t n, int d, int s, int root)
{
    const bool varying = form == F_COLLECT || form == F_COLLECTMEM;
    auto cnt = [&](int j) { return varying ? ((j % 3 == 1) ? (size_t) 0 : n + 5 * (size_t) j) : n; };
    // The PE number and the team enter the bytes: a PE of another team, running the same case at
    // the same moment, holds different ones.
    auto pat = [&](int j, size_t b) {
        return (unsigned char) (b * 7 + (size_t) (t.start + j * t.stride) * 31 + (size_t) ti * 13 + 1 + n + (size_t) form);
    };
    const size_t nbk = n * sizeof(T);
    const size_t mine = (form == F_ALLTOALL ? n * (size_t) t.size : cnt(t.me)) * sizeof(T);
    std::vector<unsigned char> src(mine), want;
    for (size_t b = 0; b < mine; ++b) src[b] = pat(t.me, b);
    if (form == F_BROADCAST || form == F_BROADCASTMEM) {
        for (size_t b = 0; b < nbk; ++b) want.push_back(pat(root, b));
    } else if (form == F_ALLTOALL) {
        for (int j = 0; j < t.size; ++j)
            for (size_t b = 0; b < nbk; ++b) want.push_back(pat(j, (size_t) t.me * nbk + b));
    } else {
        for (int j = 0; j < t.size; ++j)
            for (size_t b = 0; b < cnt(j) * sizeof(T); ++b) want.push_back(pat(j, b));
    }
    const size_t len = block_len(want.size());
    fill_block(len);
    T *dst = (T *) (db + kGuard + d);
    const T *sp = (const T *) (sb + kGuard + s);
    if (mine) (void) hipMemcpy((void *) sp, src.data(), mine, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(coll_kernel<T>, dim3(1), dim3(block), 0, 0, form, t.h, dst, sp, varying ? cnt(t.me) : n, root, rc_of(len));
    const int r = finish(len);
    const size_t bad = check_block(len, kGuard + d, want.data(), want.size());
    char op[32];
    snprintf(op, sizeof(op), "root-%d", root);
    if (r != 0 || bad) fail(kFormName[form], 0, block, t, TI<T>::name, form == F_BROADCAST || form == F_BROADCASTMEM ? op : "-", n, d, s, r, bad);
    if (r != 0) stop("a device collective returned non-zero on a member");
}

template <typename T>
static void coll_sweep(const Team &t, int ti)
{
    // uint8: odd dest offsets (the single-byte arm, local and remote); long: the 16-B and 4-B arms.
    std::vector<std::pair<int, int>> pairs;
    if (sizeof(T) == 1) pairs = {{1, 0}, {0, 0}, {3, 1}, {15, 4}};
    else pairs = {{0, 0}, {8, 8}, {8, 0}};
    std::vector<int> roots = {0};
    if (t.size > 1) roots.push_back(t.size - 1);
    int k = 0;  // block size 64 / 256 in turn (9 cases per (n, pair): every form meets both)
    for (size_t n : {(size_t) 1, (size_t) 7, (size_t) 300})
        for (const auto &p : pairs)
            for (int form = 0; form < F_COUNT; ++form) {
                if (form == F_BROADCAST || form == F_BROADCASTMEM) {
                    for (int root : roots) coll_case<T>(t, ti, form, k++ % 2 ? 256 : 64, n, p.first, p.second, root);
                } else {
                    coll_case<T>(t, ti, form, k++ % 2 ? 256 : 64, n, p.first, p.second, 0);
                }
            }
}

// A PE outside the team holds ISHMEM_TEAM_INVALID: the work-group forms return non-zero at once
// and write nothing.  (That no member is kept waiting shows in the members' own cases.)
static void nonmember_cases(const Team &t)
{
    if (t.h != ISHMEM_TEAM_INVALID) {
        if (++errors <= 16) printf("[%d] FAIL split (%d,%d,%d): a non-member got handle %d\n", g_pe, t.start, t.stride, t.size, t.h);
        return;
    }
    const size_t n = 100, len = block_len(n * 8);
    for (int k = 0; k < 3; ++k) {
        fill_block(len);
        (void) hipMemset(sb, 0x11, len);
        if (k == 0)
            hipLaunchKernelGGL((reduce_kernel<int32_t, OR_SUM>), dim3(1), dim3(64), 0, 0, t.h, (int32_t *) (db + kGuard),
                               (const int32_t *) (sb + kGuard), n, 0, rc_of(len));
        else
            hipLaunchKernelGGL(coll_kernel<long>, dim3(1), dim3(64), 0, 0, k == 1 ? F_COLLECT : F_FCOLLECT, t.h,
                               (long *) (db + kGuard), (const long *) (sb + kGuard), n, 0, rc_of(len));
        const int r = finish(len);
        const size_t bad = check_block(len, 0, nullptr, 0);
        if (r == 0 || r == kRcUnset || bad)
            fail(k == 0 ? "nonmember-reduce" : k == 1 ? "nonmember-collect" : "nonmember-fcollect", 0, 64, t,
                 k == 0 ? "int32" : "long", k == 0 ? "sum" : "-", n, 0, 0, r, bad);
    }
}

// Team queries from a kernel equal the host's answers (and the table's).
static void query_case(const Team &t)
{
    (void) hipMemset(rc, 0xff, 32 * sizeof(int));
    hipLaunchKernelGGL(query_kernel, dim3(1), dim3(1), 0, 0, t.h, t.size, rc);
    if (hipDeviceSynchronize() != hipSuccess) stop("query kernel failed");
    int q[32];
    (void) hipMemcpy(q, rc, sizeof(q), hipMemcpyDeviceToHost);
    int bad = 0;
    bad += q[0] != ishmem_team_my_pe(t.h) || q[0] != t.me;
    bad += q[1] != ishmem_team_n_pes(t.h) || q[1] != t.size;
    for (int i = 0; i <= t.size; ++i) {
        const int host = ishmem_team_translate_pe(t.h, i, ISHMEM_TEAM_WORLD);
        bad += q[2 + i] != host || host != (i < t.size ? t.start + i * t.stride : -1);
    }
    if (bad && ++errors <= 16)
        printf("[%d] FAIL device team queries team (%d,%d,%d): my_pe %d n_pes %d, %d mismatches\n", g_pe, t.start,
               t.stride, t.size, q[0], q[1], bad);
}

// Host reduce, device work-group reduce, host reduce on one team: the host and device epochs and
// flag rows are separate and must stay so.
static void interleave_case(const Team &t, int ti)
{
    const size_t n = 1000, nb = n * sizeof(int), len = block_len(nb);
    for (int step = 0; step < 3; ++step) {
        std::vector<std::vector<int>> src((size_t) t.size, std::vector<int>(n));
        std::vector<const void *> ptrs((size_t) t.size);
        for (int j = 0; j < t.size; ++j) {
            oracle_fill_random(OD_INT32, case_seed(5, ti, OD_INT32, OR_SUM, n, step, 256, 0, 0, j), 0, 0, n, src[(size_t) j].data());
            ptrs[(size_t) j] = src[(size_t) j].data();
        }
        std::vector<int> want(n);
        oracle_reduce_fold(OR_SUM, OD_INT32, ptrs.data(), t.size, 0, want.data(), n);
        fill_block(len);
        int *dst = (int *) (db + kGuard);
        const int *sp = (const int *) (sb + kGuard);
        (void) hipMemcpy((void *) sp, src[(size_t) t.me].data(), nb, hipMemcpyHostToDevice);
        int r;
        if (step == 1) {
            hipLaunchKernelGGL((reduce_kernel<int32_t, OR_SUM>), dim3(1), dim3(256), 0, 0, t.h, dst, sp, n, 0, rc_of(len));
            r = finish(len);
        } else {
            (void) hipDeviceSynchronize();
            r = ishmem_int_sum_reduce(t.h, dst, sp, n);
            (void) finish(len);
        }
        const size_t bad = check_block(len, kGuard, want.data(), nb);
        if (r != 0 || bad) fail(step == 1 ? "interleaved-device-reduce" : "interleaved-host-reduce", 0, 256, t, "int32", "sum", n, 0, 0, r, bad);
        if (r != 0) stop("an interleaved reduce returned non-zero on a member");
    }
}

int main()
{
    ishmem_init();
    const int pe = ishmem_my_pe(), npes = ishmem_n_pes();
    if (pe < 0) {
        printf("init failed: %s\n", ishmemi_c_last_error());
        return 2;
    }
    g_pe = pe;
    // Every PE calls every split; a non-member gets ISHMEM_TEAM_INVALID.
    std::vector<Team> teams = {{ISHMEM_TEAM_WORLD, 0, 1, npes, pe}};
    struct Split {
        int start, stride, size;
    };
    std::vector<Split> splits;
    if (npes == 2) splits = {{1, 1, 1}};
    else if (npes == 5) splits = {{1, 2, 2}, {0, 2, 3}};
    else if (npes == 8) splits = {{1, 2, 4}, {2, 3, 2}, {0, 1, 6}, {1, 1, 7}};
    for (const Split &sp : splits) {
        Team t{ISHMEM_TEAM_INVALID, sp.start, sp.stride, sp.size, -1};
        const int d = pe - sp.start;
        if (d >= 0 && d % sp.stride == 0 && d / sp.stride < sp.size) t.me = d / sp.stride;
        const int r = ishmem_team_split_strided(ISHMEM_TEAM_WORLD, sp.start, sp.stride, sp.size, nullptr, 0, &t.h);
        if (r != 0 || (t.me >= 0) != (t.h != ISHMEM_TEAM_INVALID)) {
            printf("[%d] FAIL split (%d,%d,%d): rc %d handle %d member %d: %s\n", pe, sp.start, sp.stride, sp.size, r, t.h,
                   t.me, ishmemi_c_last_error());
            stop("team split failed");
        }
        teams.push_back(t);
    }
    sb = (char *) ishmem_malloc(kBlk);
    db = (char *) ishmem_malloc(kBlk);
    rc = (int *) ishmem_malloc(32 * sizeof(int));
    hostblk.resize(kBlk);
    if (!sb || !db || !rc) stop("ishmem_malloc failed");

    // Teams in table order on every PE, so two PEs that share teams meet them in the same order;
    // disjoint teams (the two strided ones at 5 PEs) run their cases at the same moment.
    for (size_t ti = 0; ti < teams.size(); ++ti) {
        const Team &t = teams[ti];
        if (t.me < 0) {
            nonmember_cases(t);
            continue;
        }
        query_case(t);
        reduce_suite(t, (int) ti);
        scan_sweep<float>(t, (int) ti);
        scan_sweep<double>(t, (int) ti);
        scan_sweep<int8_t>(t, (int) ti);
        scan_sweep<uint16_t>(t, (int) ti);
        scan_sweep<int32_t>(t, (int) ti);
        scan_sweep<uint64_t>(t, (int) ti);
        scan_overlap_case(t, (int) ti);
        coll_sweep<uint8_t>(t, (int) ti);
        coll_sweep<long>(t, (int) ti);
        interleave_case(t, (int) ti);
    }

    ishmem_barrier_all();
    for (size_t ti = 1; ti < teams.size(); ++ti)
        if (teams[ti].h != ISHMEM_TEAM_INVALID) ishmem_team_destroy(teams[ti].h);
    ishmem_free(rc);
    ishmem_free(db);
    ishmem_free(sb);
    ishmem_barrier_all();
    if (ishmemi_c_error_count()) ++errors;
    printf("[%d] %s errors %d\n", pe, errors ? "FAIL" : "PASS", errors);
    ishmem_finalize();
    return errors ? 1 : 0;
}
