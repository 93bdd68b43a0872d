// The 16-bit floating-point reductions through the C++ names (include/ishmemx.h,
// include/ishmemx_device.h): half (IEEE binary16) and bfloat16 x max / min / sum / prod.
//   Forms: typed host names with and without a team, the generic host templates, the on-stream names
//   (typed, generic and with events), the _work_group forms by a thread block and by a 64-lane tile,
//   the one-work-item form; on ishmemx_half_t / ishmemx_bfloat16_t and, through the generic forms, on
//   the compiler's _Float16 / __bf16.
//   Teams: TEAM_WORLD and a strided team that starts at PE 1, so team index != PE number.
//   Sizes: 1, 9, 1027 and 192 * team size + 5 (the last chunk ends inside a 16-B item).
// Expected values: the team-order fold acc = x_0; acc = rn_T(f32(acc) OP f32(x_j)) by a host
// restatement of tests/half_model.py (float operation, integer round to nearest even), which is
// first held to triples taken from that model.  A NaN must be a NaN, everything else is bit-exact
// (the sources hold no zeros of both signs for max / min).
// Launch: ISHMEM_PE=<pe> ISHMEM_NPES=<n> ISHMEM_DEVICE=0 ISHMEM_BOOTSTRAP_KEY=<k> ./half_patterns
#include <hip/hip_cooperative_groups.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ishmem.h"
#include "ishmemx.h"

namespace cg = cooperative_groups;

static int errors = 0;
static long cases = 0;
enum { MAX = ISHMEMI_OP_MAX, MIN = ISHMEMI_OP_MIN, SUM = ISHMEMI_OP_SUM, PROD = ISHMEMI_OP_PROD };
static const char *op_name(int op) { return op == MAX ? "max" : op == MIN ? "min" : op == SUM ? "sum" : "prod"; }

// ---- the model, restated for the host --------------------------------------------------------------
static float bits_f32(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t f32_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
// kind 1: half, 2: bfloat16
static float widen(int kind, uint16_t h)
{
    if (kind == 2) return bits_f32((uint32_t) h << 16);
    const uint32_t s = (uint32_t) (h >> 15) << 31, e = (h >> 10) & 31, m = h & 1023;
    if (e == 31) return bits_f32(s | 0x7F800000u | (m << 13));
    if (e == 0) return (s ? -1.0f : 1.0f) * ldexpf((float) m, -24);  // exact
    return bits_f32(s | ((e + 112) << 23) | (m << 13));
}
static uint16_t narrow(int kind, float f)
{
    const uint32_t x = f32_bits(f), ax = x & 0x7FFFFFFFu;
    const uint16_t s = (uint16_t) ((x >> 31) << 15);
    if (kind == 2) {
        if (ax > 0x7F800000u) return (uint16_t) (s | (ax >> 16) | 0x40);
        return (uint16_t) (s | ((ax + 0x7FFFu + ((ax >> 16) & 1)) >> 16));
    }
    const uint32_t e = ax >> 23, m = ax & 0x7FFFFFu;
    if (ax > 0x7F800000u) return (uint16_t) (s | 0x7E00 | (m >> 13));
    if (ax == 0x7F800000u) return (uint16_t) (s | 0x7C00);
    if (e >= 113) {
        const uint32_t v = ax - (112u << 23);
        const uint32_t r = (v + 0xFFFu + ((v >> 13) & 1)) >> 13;
        return (uint16_t) (s | (r > 0x7C00u ? 0x7C00u : r));
    }
    if (e < 102) return s;
    const uint32_t sh = 126 - e, m24 = m | 0x800000u, q = m24 >> sh, rem = m24 & ((1u << sh) - 1), half = 1u << (sh - 1);
    return (uint16_t) (s | (q + ((rem > half) || (rem == half && (q & 1)))));
}
static bool is_nan(int kind, uint16_t h) { return (h & 0x7FFF) > (kind == 1 ? 0x7C00 : 0x7F80); }
static uint16_t model_op(int kind, int op, uint16_t a, uint16_t b)
{
    // volatile: the float operation itself, not a contracted or widened one
    volatile float x = widen(kind, a), y = widen(kind, b), r;
    if (op == MAX) r = fmaxf(x, y);
    else if (op == MIN) r = fminf(x, y);
    else if (op == SUM) r = x + y;
    else r = x * y;
    return narrow(kind, r);
}

struct Triple {
    int kind, op;
    uint16_t a, b, want;
};
static const Triple kTriples[] = {  // from tests/half_model.py binop()
    {1, SUM, 0x3C01, 0x1000, 0x3C02},  {1, SUM, 0x7BFF, 0x4C00, 0x7C00},  {1, PROD, 0x0003, 0x3800, 0x0002},
    {1, PROD, 0x3E00, 0x3C03, 0x3E04}, {1, MAX, 0x7E00, 0xBC00, 0xBC00},  {1, MIN, 0x0001, 0x8001, 0x8001},
    {2, SUM, 0x3F81, 0x3B80, 0x3F82},  {2, SUM, 0x7F7F, 0x7B00, 0x7F80},  {2, SUM, 0x7F7F, 0x7A80, 0x7F7F},
    {2, PROD, 0x0D81, 0x3081, 0x0008}, {2, PROD, 0x0003, 0x3F00, 0x0002}, {2, PROD, 0x3FC0, 0x3F83, 0x3FC4},
    {2, MAX, 0x7FC0, 0xFF80, 0xFF80},  {2, SUM, 0x0001, 0x007F, 0x0080},  {1, SUM, 0x03FF, 0x0001, 0x0400},
    {2, SUM, 0x7F80, 0xFF80, 0xFFC0},
};

// ---- sources -------------------------------------------------------------------------------------
static uint32_t mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
// Element i of team member j: mostly finite values of moderate size, every eighth a special one.
static uint16_t gen(int kind, int op, int j, size_t i)
{
    const uint32_t h = mix((uint32_t) i * 31u + (uint32_t) j * 7919u + (uint32_t) op * 104729u + (uint32_t) kind);
    const int mant = kind == 1 ? 10 : 7, bias = kind == 1 ? 15 : 127;
    const uint16_t inf = kind == 1 ? 0x7C00 : 0x7F80, one = (uint16_t) (bias << mant);
    if ((h & 7) == 0) {
        const uint16_t sp[8] = {one, 0x0000, 0x0001, (uint16_t) (inf - 1), (uint16_t) ((1u << mant) - 1), (uint16_t) (1u << mant),
                                (uint16_t) (op == MAX || op == MIN ? 0x8001 : 0x8000), (uint16_t) (inf | (op == PROD ? 0x8000 : 0))};
        const uint32_t k = (h >> 3) & 15;
        if (k == 15) return (uint16_t) (inf | (1u << (mant - 1)));  // a quiet NaN, one element in 128
        return sp[k & 7];
    }
    const int span = op == PROD ? 2 : 7;
    const uint32_t e = (uint32_t) (bias - span / 2 + (int) ((h >> 3) % (uint32_t) span));  // prod: [0.5, 2)
    return (uint16_t) (((h >> 31) << 15) | (e << mant) | ((h >> 8) & ((1u << mant) - 1)));
}

// ---- the names under test ------------------------------------------------------------------------------
#define BY_OP(OPC, PRE, POST, ...)                                                                        \
    ((OPC) == MAX ? PRE##max##POST(__VA_ARGS__) : (OPC) == MIN ? PRE##min##POST(__VA_ARGS__)                \
     : (OPC) == SUM ? PRE##sum##POST(__VA_ARGS__) : PRE##prod##POST(__VA_ARGS__))

struct K_half {
    using T = ishmemx_half_t;
    static constexpr int kind = 1;
    static const char *name() { return "half"; }
    template <int OPC> static int host(T *d, const T *s, size_t n) { return BY_OP(OPC, ishmemx_half_, _reduce, d, s, n); }
    template <int OPC> static int host(int team, T *d, const T *s, size_t n) { return BY_OP(OPC, ishmemx_half_, _reduce, team, d, s, n); }
    template <int OPC, typename... A> static int stream(A... a) { return BY_OP(OPC, ishmemx_half_, _reduce_on_stream, a...); }
    template <int OPC, typename G> __device__ static int group(int team, T *d, const T *s, size_t n, const G &g)
    {
        if (team == ISHMEM_TEAM_WORLD) return BY_OP(OPC, ishmemx_half_, _reduce_work_group, d, s, n, g);
        return BY_OP(OPC, ishmemx_half_, _reduce_work_group, team, d, s, n, g);
    }
    template <int OPC> __device__ static int item(int team, T *d, const T *s, size_t n)
    {
        if (team == ISHMEM_TEAM_WORLD) return BY_OP(OPC, ishmemx_half_, _reduce, d, s, n);
        return BY_OP(OPC, ishmemx_half_, _reduce, team, d, s, n);
    }
};
struct K_bfloat16 {
    using T = ishmemx_bfloat16_t;
    static constexpr int kind = 2;
    static const char *name() { return "bfloat16"; }
    template <int OPC> static int host(T *d, const T *s, size_t n) { return BY_OP(OPC, ishmemx_bfloat16_, _reduce, d, s, n); }
    template <int OPC> static int host(int team, T *d, const T *s, size_t n) { return BY_OP(OPC, ishmemx_bfloat16_, _reduce, team, d, s, n); }
    template <int OPC, typename... A> static int stream(A... a) { return BY_OP(OPC, ishmemx_bfloat16_, _reduce_on_stream, a...); }
    template <int OPC, typename G> __device__ static int group(int team, T *d, const T *s, size_t n, const G &g)
    {
        if (team == ISHMEM_TEAM_WORLD) return BY_OP(OPC, ishmemx_bfloat16_, _reduce_work_group, d, s, n, g);
        return BY_OP(OPC, ishmemx_bfloat16_, _reduce_work_group, team, d, s, n, g);
    }
    template <int OPC> __device__ static int item(int team, T *d, const T *s, size_t n)
    {
        if (team == ISHMEM_TEAM_WORLD) return BY_OP(OPC, ishmemx_bfloat16_, _reduce, d, s, n);
        return BY_OP(OPC, ishmemx_bfloat16_, _reduce, team, d, s, n);
    }
};
// The compiler's own types through the generic templates only.
template <typename NT, int KIND>
struct K_native {
    using T = NT;
    static constexpr int kind = KIND;
    static const char *name() { return KIND == 1 ? "_Float16" : "__bf16"; }
    template <int OPC> static int host(T *d, const T *s, size_t n) { return BY_OP(OPC, ishmem_, _reduce, d, s, n); }
    template <int OPC> static int host(int team, T *d, const T *s, size_t n) { return BY_OP(OPC, ishmem_, _reduce, team, d, s, n); }
    template <int OPC, typename... A> static int stream(A... a) { return BY_OP(OPC, ishmemx_, _reduce_on_stream, a...); }
    template <int OPC, typename G> __device__ static int group(int team, T *d, const T *s, size_t n, const G &g)
    {
        return BY_OP(OPC, ishmemx_, _reduce_work_group, team, d, s, n, g);
    }
    template <int OPC> __device__ static int item(int team, T *d, const T *s, size_t n) { return BY_OP(OPC, ishmem_, _reduce, team, d, s, n); }
};
static_assert(ishmemi_cxx::dtype_of<__half>() == ISHMEMI_DT_HALF && ishmemi_cxx::dtype_of<_Float16>() == ISHMEMI_DT_HALF, "half");
static_assert(ishmemi_cxx::dtype_of<__hip_bfloat16>() == ISHMEMI_DT_BFLOAT16 && ishmemi_cxx::dtype_of<__bf16>() == ISHMEMI_DT_BFLOAT16,
              "bfloat16");
static_assert(sizeof(ishmemx_half_t) == 2 && sizeof(ishmemx_bfloat16_t) == 2, "2-byte storage");

enum Form { kHost = 0, kHostGeneric, kOnStream, kOnStreamEvents, kBlock, kTile, kItem, kForms };
static const char *const kFormName[kForms] = {"host", "host generic", "on_stream", "on_stream events", "work_group block",
                                              "work_group tile64", "one work-item"};

template <typename K, int OPC, int FORM>
__global__ void dev_kernel(int team, typename K::T *d, const typename K::T *s, size_t n, int *rc)
{
    if constexpr (FORM == kBlock) {
        const int r = K::template group<OPC>(team, d, s, n, cg::this_thread_block());
        if (threadIdx.x == 0) *rc = r;
    } else if constexpr (FORM == kTile) {
        auto tile = cg::tiled_partition<64>(cg::this_thread_block());
        if (threadIdx.x / 64 != 1) return;  // only the second wavefront takes part
        const int r = K::template group<OPC>(team, d, s, n, tile);
        if (tile.thread_rank() == 0) *rc = r;
    } else {
        if (threadIdx.x != 0) return;
        *rc = K::template item<OPC>(team, d, s, n);
    }
}

struct TeamInfo {
    int handle;
    std::vector<int> members;  // global PE of every team index
    int my_idx;                // -1: not a member
    const char *name;
};

template <typename K, int OPC>
static void one_case(const TeamInfo &t, int form, size_t n, char *sb, char *db, int *rc, hipStream_t st, hipEvent_t ev[2])
{
    using T = typename K::T;
    const int pe = ishmem_my_pe(), p = (int) t.members.size();
    ++cases;
    std::vector<uint16_t> want(n), got(n + 16), mine(n);
    for (size_t i = 0; i < n; ++i) {
        uint16_t acc = gen(K::kind, OPC, 0, i);
        for (int j = 1; j < p; ++j) acc = model_op(K::kind, OPC, acc, gen(K::kind, OPC, j, i));
        want[i] = acc;
        if (t.my_idx >= 0) mine[i] = gen(K::kind, OPC, t.my_idx, i);
    }
    (void) hipMemcpy(sb, mine.data(), n * 2, hipMemcpyHostToDevice);
    (void) hipMemset(db, 0xA5, n * 2 + 32);
    (void) hipMemset(rc, 0xFF, sizeof(int));
    (void) hipDeviceSynchronize();
    ishmem_barrier_all();  // every member's source is in place; non-members only join the barriers
    if (t.my_idx >= 0) {
        T *d = (T *) db;
        const T *s = (const T *) sb;
        const bool world = t.handle == ISHMEM_TEAM_WORLD;
        int r = 0, dev_rc = 0;
        switch (form) {
            case kHost: r = world ? K::template host<OPC>(d, s, n) : K::template host<OPC>(t.handle, d, s, n); break;
            case kHostGeneric: r = BY_OP(OPC, ishmem_, _reduce, t.handle, d, s, n); break;
            case kOnStream:
                r = world ? K::template stream<OPC>(d, s, n, rc, st) : K::template stream<OPC>(t.handle, d, s, n, rc, st);
                (void) hipStreamSynchronize(st);
                break;
            case kOnStreamEvents:
                (void) hipEventRecord(ev[0], st);
                r = K::template stream<OPC>(t.handle, d, s, n, rc, st, (const hipEvent_t *) &ev[0], (size_t) 1, ev[1]);
                (void) hipEventSynchronize(ev[1]);
                break;
            case kBlock: hipLaunchKernelGGL((dev_kernel<K, OPC, kBlock>), dim3(1), dim3(256), 0, 0, t.handle, d, s, n, rc); break;
            case kTile: hipLaunchKernelGGL((dev_kernel<K, OPC, kTile>), dim3(1), dim3(128), 0, 0, t.handle, d, s, n, rc); break;
            default: hipLaunchKernelGGL((dev_kernel<K, OPC, kItem>), dim3(1), dim3(64), 0, 0, t.handle, d, s, n, rc); break;
        }
        (void) hipDeviceSynchronize();
        if (form >= kOnStream) (void) hipMemcpy(&dev_rc, rc, sizeof(int), hipMemcpyDeviceToHost);
        (void) hipMemcpy(got.data(), db, got.size() * 2, hipMemcpyDeviceToHost);
        size_t bad = 0, first = n;
        for (size_t i = 0; i < n; ++i) {
            const bool ok = is_nan(K::kind, want[i]) ? is_nan(K::kind, got[i]) : got[i] == want[i];
            if (!ok && first == n) first = i;
            bad += !ok;
        }
        size_t guard = 0;
        for (size_t i = n; i < got.size(); ++i) guard += got[i] != 0xA5A5;
        if (r != 0 || dev_rc != 0 || bad || guard) {
            if (++errors <= 16)
                printf("[%d] FAIL %s %s %s team %s n %zu: rc %d / %d, %zu wrong (first %zu: got %#06x want %#06x), %zu guard "
                       "words written: %s\n", pe, K::name(), op_name(OPC), kFormName[form], t.name, n, r, dev_rc, bad, first,
                       first < n ? got[first] : 0, first < n ? want[first] : 0, guard, ishmemi_c_last_error());
        }
    }
    ishmem_barrier_all();  // nobody overwrites a source a member still reads
}

template <typename K>
static void all_cases(const std::vector<TeamInfo> &teams, bool native, char *sb, char *db, int *rc, hipStream_t st,
                      hipEvent_t ev[2])
{
    for (const TeamInfo &t : teams) {
        const size_t derived = 192 * t.members.size() + 5;
        for (size_t n : {(size_t) 1, (size_t) 9, (size_t) 1027, derived}) {
            for (int form = 0; form < kForms; ++form) {
                // the compiler's types: the generic forms only, at one small and the derived size
                if (native && (form == kHost || form == kOnStreamEvents || n == 1 || n == 1027)) continue;
                one_case<K, MAX>(t, form, n, sb, db, rc, st, ev);
                one_case<K, MIN>(t, form, n, sb, db, rc, st, ev);
                one_case<K, SUM>(t, form, n, sb, db, rc, st, ev);
                one_case<K, PROD>(t, form, n, sb, db, rc, st, ev);
            }
        }
    }
}

int main()
{
    for (const Triple &t : kTriples) {
        const uint16_t got = model_op(t.kind, t.op, t.a, t.b);
        if (got != t.want && ++errors <= 16)
            printf("FAIL host model: kind %d %s %#06x %#06x = %#06x, the Python model has %#06x\n", t.kind, op_name(t.op), t.a,
                   t.b, got, t.want);
    }
    for (int kind = 1; kind <= 2; ++kind)
        for (uint32_t h = 0; h < 65536; ++h)
            if (!is_nan(kind, (uint16_t) h) && narrow(kind, widen(kind, (uint16_t) h)) != h && ++errors <= 16)
                printf("FAIL host model: kind %d %#06x does not survive widen / narrow\n", kind, h);
    ishmem_init();
    const int pe = ishmem_my_pe(), npes = ishmem_n_pes();
    if (pe < 0) {
        printf("init failed: %s\n", ishmemi_c_last_error());
        return 2;
    }
    const size_t maxn = 4096;
    char *sb = (char *) ishmem_malloc(maxn * 2);
    char *db = (char *) ishmem_malloc(maxn * 2 + 64);
    int *rc = (int *) ishmem_malloc(sizeof(int));
    hipStream_t st;
    hipEvent_t ev[2];
    (void) hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    (void) hipEventCreate(&ev[0]);
    (void) hipEventCreate(&ev[1]);

    std::vector<TeamInfo> teams;
    TeamInfo world{ISHMEM_TEAM_WORLD, {}, pe, "world"};
    for (int j = 0; j < npes; ++j) world.members.push_back(j);
    teams.push_back(world);
    // A strided team that starts at PE 1: team index != PE number (PEs 1, 2 at 3 PEs; 1, 3 at 5).
    const int start = 1, stride = npes >= 5 ? 2 : 1, size = npes >= 5 ? 2 : npes - 1;
    TeamInfo sub{ISHMEM_TEAM_INVALID, {}, -1, "strided from PE 1"};
    if (ishmem_team_split_strided(ISHMEM_TEAM_WORLD, start, stride, size, nullptr, 0, &sub.handle) != 0) {
        ++errors;
        printf("[%d] FAIL team split: %s\n", pe, ishmemi_c_last_error());
    }
    for (int j = 0; j < size; ++j) {
        sub.members.push_back(start + j * stride);
        if (start + j * stride == pe) sub.my_idx = j;
    }
    if ((sub.my_idx >= 0) != (sub.handle != ISHMEM_TEAM_INVALID)) {
        ++errors;
        printf("[%d] FAIL team split: handle %d, member index %d\n", pe, sub.handle, sub.my_idx);
        sub.my_idx = -1;
    }
    teams.push_back(sub);

    all_cases<K_half>(teams, false, sb, db, rc, st, ev);
    all_cases<K_bfloat16>(teams, false, sb, db, rc, st, ev);
    all_cases<K_native<_Float16, 1>>(teams, true, sb, db, rc, st, ev);
    all_cases<K_native<__bf16, 2>>(teams, true, sb, db, rc, st, ev);

    if (sub.handle != ISHMEM_TEAM_INVALID) ishmem_team_destroy(sub.handle);
    (void) hipEventDestroy(ev[0]);
    (void) hipEventDestroy(ev[1]);
    (void) hipStreamDestroy(st);
    ishmem_free(rc);
    ishmem_free(db);
    ishmem_free(sb);
    ishmem_barrier_all();
    if (ishmemi_c_error_count()) ++errors;
    printf("[%d] %s errors %d (%ld cases)\n", pe, errors ? "FAIL" : "PASS", errors, cases);
    ishmem_finalize();
    return errors ? 1 : 0;
}
