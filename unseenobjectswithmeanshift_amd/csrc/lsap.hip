// The set criterion's assignments on the device: the rectangular linear sum assignment of every (prediction, image) cost matrix
// that msm_match_cost wrote, solved where it lies, so that a criterion call never waits for the GPU.
//
//   lsap_kernel   one workgroup of ONE wave per problem (p, b); the grid is n_pred * B.  Shortest augmenting paths (Crouse 2016,
//                 the algorithm of scipy's linear_sum_assignment) exactly as criterion.lsap_numpy states it: float64 arithmetic on
//                 the upcast fp32 costs in lsap_numpy's operation order (additions and subtractions only, so there is nothing to
//                 contract), iteration over the smaller side, and its tie rule -- among the unseen columns of least `shortest`
//                 the lowest unassigned one, else the lowest -- as one lexicographic arg-min over (value, assigned, column).
//
// Why one wave.  A column selection is a scan of nc <= 1024 columns (at most 16 per lane) followed by one arg-min over the
// workgroup, and the selections of a problem are a dependent chain.  Within a wave the arg-min is six register butterfly stages
// (v_permlane32/16_swap, DPP) of three words each and needs no barrier; with more waves every selection would add an LDS
// exchange and two barriers, more than the lanes they bring save on a scan of two to five columns per lane at the criterion's
// sizes (Q = 100 .. 300).  The parallelism is across the n_pred * B problems.
//
// No workgroup talks to another: no atomics, no spins, no persistent structure.  Every loop is counted (augmentations <= nr,
// column selections <= nc per augmentation, path unwinding <= nr steps); running past a bound sets status 3 and leaves.  Any
// non-zero status ends in the fallback pairs (q = j, target j), so whatever reads `pairs` next stays in bounds.
#include "common.h"

#include <math.h>

namespace {

using namespace msm;

constexpr int LS_MAX = MSM_LSAP_MAX_DIM;     // rows / columns of one problem
constexpr int LS_LANES = 64;
constexpr int LS_STAGE_MAX = 28672;          // fp32 values of one staged working matrix (112 KiB next to 38 KiB of state)
constexpr unsigned LS_ASSIGNED = 1u << 30;   // tag = (assigned ? LS_ASSIGNED : 0) | column
constexpr unsigned LS_NONE = 0xffffffffu;    // tag of a lane without an unseen column

// (value, tag): value as the order-preserving 64-bit image of a double (hi, lo), compared lexicographically
struct LsKey {
    unsigned lo, hi, tag;
};

__device__ __forceinline__ bool ls_less(const LsKey& a, const LsKey& b) {
    if (a.hi != b.hi) return a.hi < b.hi;
    if (a.lo != b.lo) return a.lo < b.lo;
    return a.tag < b.tag;
}

// the smaller of two keys, word by word (a select per word keeps the key in registers)
__device__ __forceinline__ LsKey ls_min(const LsKey& a, const LsKey& b) {
    const bool l = ls_less(b, a);
    LsKey r;
    r.lo = l ? b.lo : a.lo;
    r.hi = l ? b.hi : a.hi;
    r.tag = l ? b.tag : a.tag;
    return r;
}

// a < b as doubles  <=>  ls_order(a) < ls_order(b) as unsigned (no nan; -0 counts as +0, as in numpy's `vals == lowest`)
__device__ __forceinline__ unsigned long long ls_order(double x) {
    unsigned long long b = (unsigned long long)__double_as_longlong(x);
    if (b == 0x8000000000000000ull) b = 0;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ls_value(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// the least key of the wave in every lane: butterfly over lane ^ 32, 16 (v_permlane*_swap hands every lane its own and its
// partner's word), then 8, 4, 2, 1 inside the 16-lane rows (DPP)
__device__ __forceinline__ LsKey ls_wave_argmin(LsKey k) {
    typedef unsigned u32x2s __attribute__((ext_vector_type(2)));
    {
        const u32x2s a = __builtin_amdgcn_permlane32_swap(k.lo, k.lo, false, false), b = __builtin_amdgcn_permlane32_swap(k.hi, k.hi, false, false),
                     c = __builtin_amdgcn_permlane32_swap(k.tag, k.tag, false, false);
        const LsKey x = {a.x, b.x, c.x}, y = {a.y, b.y, c.y};
        k = ls_min(x, y);
    }
    {
        const u32x2s a = __builtin_amdgcn_permlane16_swap(k.lo, k.lo, false, false), b = __builtin_amdgcn_permlane16_swap(k.hi, k.hi, false, false),
                     c = __builtin_amdgcn_permlane16_swap(k.tag, k.tag, false, false);
        const LsKey x = {a.x, b.x, c.x}, y = {a.y, b.y, c.y};
        k = ls_min(x, y);
    }
#define LS_STAGE(FN)                                                                                          \
    {                                                                                                         \
        const LsKey o = {__float_as_uint(FN(__uint_as_float(k.lo))), __float_as_uint(FN(__uint_as_float(k.hi))), \
                         __float_as_uint(FN(__uint_as_float(k.tag)))};                                        \
        k = ls_min(k, o);                                                                                    \
    }
    LS_STAGE(wave_xor_dpp8)
    LS_STAGE(wave_xor_dpp4)
    LS_STAGE(wave_xor_dpp2)
    LS_STAGE(wave_xor_dpp1)
#undef LS_STAGE
    return k;
}

__global__ __launch_bounds__(LS_LANES) void lsap_kernel(const float* __restrict__ cost, const int64_t* __restrict__ table,
                                                        const int32_t* __restrict__ labels, int32_t* __restrict__ pairs,
                                                        int64_t* __restrict__ target_classes, int32_t* __restrict__ status, int B, int Q,
                                                        int TT, int N, int no_object, int staged) {
    extern __shared__ float ls_m[];          // the working matrix [nr][nc] when `staged`
    __shared__ double s_u[LS_MAX], s_v[LS_MAX], s_shortest[LS_MAX];
    __shared__ int s_path[LS_MAX], s_row4col[LS_MAX], s_col4row[LS_MAX];
    __shared__ unsigned char s_seen[LS_MAX]; // seen columns; the seen rows are `cur` and row4col of the seen columns

    const int lane = threadIdx.x;
    const int p = blockIdx.x / B, b = blockIdx.x % B;
    const int64_t toff = table[b], poff = table[B + 1 + b];
    const int64_t Tl = table[b + 1] - toff;
    if (Tl < 0 || Tl > LS_MAX || toff < 0 || toff + Tl > TT) {      // a table the wrapper would never build
        if (lane == 0) status[blockIdx.x] = 3;
        return;
    }
    const int T = (int)Tl;
    const bool transpose = T < Q;
    const int nr = transpose ? T : Q, nc = transpose ? Q : T;       // nr <= nc: the solver iterates over the smaller side
    const float* cp = cost + (int64_t)p * Q * TT + toff;            // cost[p][q][toff + t] = cp[q * TT + t]

    // stage (transposed where needed) and look for nan / -inf on the way
    bool bad = false;
    for (int e = lane; e < Q * T; e += LS_LANES) {
        const int q = e / T, t = e - q * T;
        const float c = cp[(int64_t)q * TT + t];
        bad |= (c != c) || (c == -INFINITY);
        if (staged) ls_m[transpose ? t * nc + q : e] = c;
    }
    int st = __ballot(bad) != 0ull ? 1 : 0;
    for (int i = lane; i < nr; i += LS_LANES) s_u[i] = 0.0, s_col4row[i] = -1;
    for (int j = lane; j < nc; j += LS_LANES) s_v[j] = 0.0, s_row4col[j] = -1;
    __syncthreads();

    const int64_t rs = transpose ? 1 : TT, cs = transpose ? TT : 1; // strides of the working matrix in `cost`
    for (int cur = 0; cur < nr && st == 0; ++cur) {
        for (int j = lane; j < nc; j += LS_LANES) s_shortest[j] = INFINITY, s_path[j] = -1, s_seen[j] = 0;
        double min_val = 0.0;
        int i = cur, sink = -1;
        for (int step = 0; step < nc; ++step) {                     // every selection marks a new column: at most nc
            const double ui = s_u[i];
            LsKey best = {LS_NONE, LS_NONE, LS_NONE};
            for (int j = lane; j < nc; j += LS_LANES) {
                if (s_seen[j]) continue;
                const double c = (double)(staged ? ls_m[i * nc + j] : cp[i * rs + j * cs]);
                const double r = ((min_val + c) - ui) - s_v[j];
                double sh = s_shortest[j];
                if (r < sh) {
                    sh = r;
                    s_shortest[j] = r;
                    s_path[j] = i;
                }
                const unsigned long long o = ls_order(sh);
                const LsKey k = {(unsigned)o, (unsigned)(o >> 32), (s_row4col[j] >= 0 ? LS_ASSIGNED : 0u) | (unsigned)j};
                best = ls_min(best, k);
            }
            best = ls_wave_argmin(best);
            if (best.tag == LS_NONE) {                              // no unseen column left: unreachable
                st = 3;
                break;
            }
            const double lowest = ls_value(((unsigned long long)best.hi << 32) | best.lo);
            if (!(lowest < (double)INFINITY)) {                     // lsap_numpy: "cost matrix is infeasible"
                st = 2;
                break;
            }
            const int j = (int)(best.tag & (LS_ASSIGNED - 1));      // a column this wave scanned: j < nc
            min_val = lowest;
            s_seen[j] = 1;                                          // every lane writes the same value
            const int r4 = s_row4col[j];
            if (r4 < 0) {
                sink = j;
                break;
            }
            i = r4;
        }
        if (st == 0 && sink < 0) st = 3;
        if (st != 0) break;

        // dual updates: u[cur] += min_val; the other seen rows are row4col of the seen columns (the sink's is free)
        if (lane == 0) s_u[cur] += min_val;
        for (int j = lane; j < nc; j += LS_LANES) {
            if (!s_seen[j]) continue;
            const double d = min_val - s_shortest[j];
            const int r4 = s_row4col[j];
            if (r4 >= 0) s_u[r4] += d;
            s_v[j] -= d;
        }
        __syncthreads();

        // augment along the path, the same in every lane
        int j = sink;
        bool done = false;
        for (int step = 0; step < nr; ++step) {
            if (j < 0 || j >= nc) break;
            const int pi = s_path[j];
            if (pi < 0 || pi >= nr) break;
            s_row4col[j] = pi;
            const int next = s_col4row[pi];
            s_col4row[pi] = j;
            j = next;
            if (pi == cur) {
                done = true;
                break;
            }
        }
        if (!done) st = 3;
        __syncthreads();
    }

    // target of every query: row4col when the rows are targets, col4row when they are queries; both hold Q entries
    int* tq = transpose ? s_row4col : s_col4row;
    if (st != 0) {
        __syncthreads();
        for (int q = lane; q < Q; q += LS_LANES) tq[q] = q < nr ? q : -1;
        __syncthreads();
    }
    if (lane == 0) status[blockIdx.x] = st;

    int4* out = reinterpret_cast<int4*>(pairs) + ((int64_t)p * N + poff);
    int64_t* tc = target_classes + (int64_t)blockIdx.x * Q;
    int base = 0;
    for (int q0 = 0; q0 < Q; q0 += LS_LANES) {
        const int q = q0 + lane;
        int t = q < Q ? tq[q] : -1;
        if (t >= T) t = -1;
        if (q < Q) tc[q] = t >= 0 ? (int64_t)labels[toff + t] : (int64_t)no_object;
        const unsigned long long m = __ballot(t >= 0);
        const int n = base + __popcll(m & ((1ull << lane) - 1ull));
        if (t >= 0 && n < nr) out[n] = make_int4(p, (int)poff + n, b * Q + q, (int)toff + t);
        base += __popcll(m);
    }
}

}  // namespace

extern "C" int msm_lsap_match(const float* cost, const int64_t* table, const int32_t* labels, int32_t* pairs, int64_t* target_classes,
                              int32_t* status, int n_pred, int B, int Q, int TT, int max_T, int N, int no_object, void* stream) {
    MSM_REQUIRE(n_pred >= 1 && B >= 0 && Q >= 1 && TT >= 0 && max_T >= 0 && max_T <= TT && N >= 0,
                "msm_lsap_match: bad sizes n_pred=%d B=%d Q=%d TT=%d max_T=%d N=%d", n_pred, B, Q, TT, max_T, N);
    MSM_REQUIRE(Q <= LS_MAX && max_T <= LS_MAX, "msm_lsap_match: Q=%d / max_T=%d exceed the supported %d", Q, max_T, LS_MAX);
    MSM_REQUIRE((int64_t)n_pred * B < (1ll << 31) && (int64_t)n_pred * N < (1ll << 29),
                "msm_lsap_match: n_pred=%d B=%d N=%d exceed the grid", n_pred, B, N);
    if (B == 0) return MSM_OK;
    MSM_REQUIRE(table && target_classes && status, "msm_lsap_match: null pointer");
    MSM_REQUIRE(TT == 0 || (cost && labels), "msm_lsap_match: null cost or labels pointer");
    MSM_REQUIRE(N == 0 || (pairs && ((uintptr_t)pairs & 15) == 0), "msm_lsap_match: pairs must be a 16-byte aligned pointer");
    const int64_t vals = (int64_t)Q * max_T;
    const int staged = vals <= LS_STAGE_MAX ? 1 : 0;
    const size_t lds = staged ? (size_t)vals * sizeof(float) : 0;
    if (lds) MSM_CHECK_HIP((hipError_t)msm::ensure_dynamic_lds((const void*)lsap_kernel, lds));
    hipLaunchKernelGGL(lsap_kernel, dim3((unsigned)(n_pred * B)), dim3(LS_LANES), lds, (hipStream_t)stream, cost, table, labels, pairs,
                       target_classes, status, B, Q, TT, N, no_object, staged);
    MSM_CHECK_LAUNCH("msm_lsap_match");
    return MSM_OK;
}
