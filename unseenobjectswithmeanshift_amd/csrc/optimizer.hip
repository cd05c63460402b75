// AdamW, Adam and SGD behind clip_grad_norm_ over a device-resident table of tensors, with GradScaler's fused protocol inside the
// launches (see include/msm_hip.h: msm_optim_count_norm, msm_optim_update, msm_optim_zero).  Reference: Trainer.build_optimizer,
// MSMFormer/tabletop_train_net_pretrained.py:113-191 -- torch.nn.utils.clip_grad_norm_ over every parameter followed by
// torch.optim.AdamW with one param group per tensor -- and torch.optim.Adam / SGD of tools/train_net.py:130-142.
//
// The table cuts every tensor into chunks of OPT_CHUNK elements (a 3-element bias is one chunk, a 524 288-element weight 64), and a
// launch is one workgroup per chunk, whatever the number of tensors:
//   norm    workgroup c: sum of g^2 over its chunk, in double -> partials[c]; the workgroup of a tensor's first chunk counts its step
//   update  workgroup c: adds partials[0 .. n_chunks) (thread t takes t, t + 256, ... in ascending order, then a fixed tree over the
//           256 threads: every workgroup forms the same bits), total_norm and coef from it, then the rule's update of its chunk
//   zero    workgroup c: g = 0 over its chunk
// A third launch that sums the partials once would save every workgroup n_chunks L2 reads of 8 bytes (about 17 KiB for the 298
// tensors of the ResNet-50 head, against the 288 KiB of HBM traffic of a full chunk) and cost a launch and a dependent kernel
// boundary on a step that is two launches and 0.1 ms long.
// The step count of a tensor is written by the norm launch (or the one-thread-per-record count launch that stands in for it when
// nothing is clipped) and only read by the update launch behind it on the stream.  The gradient is unscaled and the step skipped
// inside the launches (GradScaler's grad_scale / found_inf).  No atomics, no hand-off between workgroups: bit-identical from call
// to call for a given table.
#include "common.h"

namespace msm {

constexpr int OPT_T = 256;                  // threads per workgroup
constexpr int OPT_CHUNK = MSM_OPTIM_CHUNK;  // elements per chunk (a multiple of 4 OPT_T: whole float4 rounds)
constexpr int OPT_REC = 8;                  // int64 per tensor record
constexpr int OPT_HYP = 8;                  // doubles per hyper-parameter row
static_assert(OPT_CHUNK % (4 * OPT_T) == 0, "a chunk is whole float4 rounds of the workgroup");

struct OptChunk {
    float *p, *g, *m, *v;
    int n;                                  // elements of this chunk (0: a record the kernel refuses)
    int row;
    bool vec;                               // 16-byte accesses
};

// chunk c of the table.  A tensor index, an offset or a row outside the table gives n = 0: the table is written by the host, and a
// stale or torn one must end as a skipped chunk, not as a wild access.
__device__ __forceinline__ OptChunk opt_chunk(const int64_t* __restrict__ tensors, const int64_t* __restrict__ chunks, int c, int n_tensors,
                                              int n_rows, int64_t align_bit) {
    OptChunk k;
    const int64_t t = chunks[2 * (int64_t)c], off = chunks[2 * (int64_t)c + 1];
    k.n = 0;
    k.row = 0;
    k.vec = false;
    k.p = k.g = k.m = k.v = nullptr;
    if (t < 0 || t >= n_tensors) return k;
    const int64_t* r = tensors + t * OPT_REC;
    const int64_t numel = r[4], row = r[5];
    if (off < 0 || off >= numel || (off & 3) || row < 0 || row >= n_rows) return k;
    k.p = reinterpret_cast<float*>(r[0]) + off;
    k.g = reinterpret_cast<float*>(r[1]) + off;
    k.m = reinterpret_cast<float*>(r[2]) + off;
    k.v = reinterpret_cast<float*>(r[3]) + off;
    k.n = (int)min((int64_t)OPT_CHUNK, numel - off);
    k.row = (int)row;
    k.vec = (r[6] & align_bit) != 0;
    return k;
}

// sum over the workgroup in a fixed tree; every thread gets it
__device__ __forceinline__ double opt_block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = OPT_T / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(OPT_T) void optim_zero_kernel(const int64_t* __restrict__ tensors, const int64_t* __restrict__ chunks, int n_tensors) {
    const int tid = threadIdx.x, c = blockIdx.x;
    const OptChunk k = opt_chunk(tensors, chunks, c, n_tensors, INT32_MAX, MSM_OPTIM_ALIGNED_G);
    if (k.vec) {
        const int n4 = k.n & ~3;
        for (int i = tid * 4; i < n4; i += OPT_T * 4) *reinterpret_cast<float4*>(k.g + i) = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n4 + tid < k.n) k.g[n4 + tid] = 0.f;
    } else {
        for (int i = tid; i < k.n; i += OPT_T) k.g[i] = 0.f;
    }
}

// *found_inf != 0 (a nan too): the step is not taken.  The same word for every workgroup of both launches of a step.
__device__ __forceinline__ bool opt_skipped(const float* __restrict__ found_inf) { return found_inf != nullptr && !(*found_inf == 0.f); }

// 1 / scale in double, rounded once: exact for GradScaler's powers of two (grad_scaler.py:336 forms the same number)
__device__ __forceinline__ float opt_inv_scale(const float* __restrict__ grad_scale) {
    return grad_scale != nullptr ? (float)(1.0 / (double)*grad_scale) : 1.f;
}

__global__ __launch_bounds__(OPT_T) void optim_count_norm_kernel(const int64_t* __restrict__ tensors, const int64_t* __restrict__ chunks,
                                                                 double* __restrict__ partials, int64_t* __restrict__ steps,
                                                                 const float* __restrict__ grad_scale, const float* __restrict__ found_inf,
                                                                 int n_tensors, int n_rows) {
    __shared__ double red[OPT_T];
    const int tid = threadIdx.x, c = blockIdx.x;
    const OptChunk k = opt_chunk(tensors, chunks, c, n_tensors, n_rows, MSM_OPTIM_ALIGNED_G);
    const bool scaled = grad_scale != nullptr;
    const float inv = opt_inv_scale(grad_scale);
    double acc = 0.0;
    if (k.vec) {
        const int n4 = k.n & ~3;
        for (int i = tid * 4; i < n4; i += OPT_T * 4) {
            float4 g = *reinterpret_cast<const float4*>(k.g + i);
            if (scaled) g.x *= inv, g.y *= inv, g.z *= inv, g.w *= inv;
            acc = fma((double)g.x, (double)g.x, acc);
            acc = fma((double)g.y, (double)g.y, acc);
            acc = fma((double)g.z, (double)g.z, acc);
            acc = fma((double)g.w, (double)g.w, acc);
        }
        if (n4 + tid < k.n) {
            float g = k.g[n4 + tid];
            if (scaled) g *= inv;
            acc = fma((double)g, (double)g, acc);
        }
    } else {
        for (int i = tid; i < k.n; i += OPT_T) {
            float g = k.g[i];
            if (scaled) g *= inv;
            acc = fma((double)g, (double)g, acc);
        }
    }
    const double s = opt_block_sum(acc, red);
    if (tid == 0) {
        partials[c] = s;
        // the workgroup of a tensor's first chunk counts its step: one writer per count, read by the update launch behind this one
        if (k.n > 0 && chunks[2 * (int64_t)c + 1] == 0 && !opt_skipped(found_inf)) steps[k.row] += 1;
    }
}

// max_norm <= 0: no norm launch, the counts move in this one (thread t: record t)
__global__ __launch_bounds__(OPT_T) void optim_count_kernel(const int64_t* __restrict__ tensors, int64_t* __restrict__ steps,
                                                            const float* __restrict__ found_inf, int n_tensors, int n_rows) {
    const int t = blockIdx.x * OPT_T + threadIdx.x;
    if (t >= n_tensors || opt_skipped(found_inf)) return;
    const int64_t* r = tensors + (int64_t)t * OPT_REC;
    const int64_t numel = r[4], row = r[5];
    if (numel < 1 || row < 0 || row >= n_rows) return;          // what opt_chunk refuses for the chunk at offset 0
    steps[row] += 1;
}

struct OptScalars {                          // of one hyper row and step, prepared once per workgroup in double
    float coef, inv_scale;
    float decay, w1, b2, w2, bc2s, eps, step_size;          // AdamW and Adam (Adam: without decay)
    float wd, lr, momentum, undamped;                       // Adam and SGD add wd p to the gradient; the rest is SGD's
    int first, nesterov;
};

// The access path of an element: the scalar loop (a tensor that is not 16-byte aligned), the 16-byte loop, the numel % 4 tail behind it
constexpr int OPT_FORM_SCALAR = 0, OPT_FORM_VEC = 1, OPT_FORM_TAIL = 2;

// One element of a rule.  Contraction is off: every operation below is rounded on its own unless it is written as an fma.
// AdamW's arithmetic is defined per access path, and the three forms are this project's AdamW (include/msm_hip.h states them;
// tests/golden/optim_adamw_bits.json pins their bits):
//   OPT_FORM_SCALAR  no fma
//   OPT_FORM_VEC     m, v and p fused
//   OPT_FORM_TAIL    m alone fused
// Adam and SGD have one form, without an fma: the compiler's choice of which products to fuse may not differ between the loops, or
// between a scaled and an unscaled step.
template <int RULE, int FORM>
__device__ __forceinline__ void opt_rule_update(float& p, float& g, float& m, float& v, const OptScalars& s, bool unscale, bool clip) {
#pragma clang fp contract(off)
    if (unscale) g = g * s.inv_scale;
    if (clip) g = g * s.coef;
    if (RULE == MSM_OPTIM_ADAMW) {
        const float d = g - m, gg = s.w2 * g, vb = v * s.b2;
        m = FORM == OPT_FORM_SCALAR ? m + d * s.w1 : __builtin_fmaf(s.w1, d, m);
        v = FORM == OPT_FORM_VEC ? __builtin_fmaf(g, gg, vb) : vb + gg * g;
        const float q = s.step_size * (m / (sqrtf(v) / s.bc2s + s.eps));
        p = FORM == OPT_FORM_VEC ? __builtin_fmaf(s.decay, p, -q) : p * s.decay - q;
        return;
    }
    float d = g;                                // g + wd p is not written back
    if (s.wd != 0.f) d = g + s.wd * p;
    if (RULE == MSM_OPTIM_ADAM) {
        m += (d - m) * s.w1;
        v = v * s.b2 + s.w2 * d * d;
        p -= s.step_size * (m / (sqrtf(v) / s.bc2s + s.eps));
    } else {
        if (s.momentum != 0.f) {
            m = s.first ? d : s.momentum * m + s.undamped * d;
            d = s.nesterov ? d + s.momentum * m : m;
        }
        p -= s.lr * d;
    }
}

template <int RULE>
__global__ __launch_bounds__(OPT_T) void optim_update_kernel(const int64_t* __restrict__ tensors, const int64_t* __restrict__ chunks,
                                                             const double* __restrict__ hyper, const double* __restrict__ partials,
                                                             int64_t* __restrict__ state, const int64_t* __restrict__ steps,
                                                             const float* __restrict__ grad_scale, const float* __restrict__ found_inf,
                                                             int n_tensors, int n_chunks, int n_rows, float max_norm) {
    __shared__ double red[OPT_T];
    __shared__ OptScalars sh;
    if (opt_skipped(found_inf)) return;         // the whole grid alike: p, the state, .grad and the state block stay as they are
    const int tid = threadIdx.x, c = blockIdx.x;
    OptChunk k = opt_chunk(tensors, chunks, c, n_tensors, n_rows, MSM_OPTIM_ALIGNED);
    const double* h = hyper + (int64_t)k.row * OPT_HYP;
    constexpr bool USE_V = RULE != MSM_OPTIM_SGD;
    const bool use_m = RULE != MSM_OPTIM_SGD || h[5] != 0.0;
    if (k.n > 0) {                              // a record without the state its rule needs is refused: the addresses of the record
        const int64_t* r = tensors + chunks[2 * (int64_t)c] * OPT_REC;          // itself, k.m and k.v are offset by the chunk
        if ((use_m && r[2] == 0) || (USE_V && r[3] == 0)) k.n = 0;
    }
    double total = 0.0, coef = 1.0;
    if (max_norm > 0.f) {
        double a = 0.0;
        for (int j = tid; j < n_chunks; j += OPT_T) a += partials[j];
        total = sqrt(opt_block_sum(a, red));
        const double q = (double)max_norm / (total + 1e-6);
        coef = q > 1.0 ? 1.0 : q;               // a nan norm stays a nan coefficient, as torch's clamp(max=1) leaves it
    }
    if (tid == 0) {
        const double lr = h[0], wd = h[1], b1 = h[2], b2 = h[3], eps = h[4];
        const int64_t count = steps[k.row];
        OptScalars s;
        s.coef = (float)coef;
        s.inv_scale = opt_inv_scale(grad_scale);
        s.decay = (float)(1.0 - lr * wd);
        s.w1 = (float)(1.0 - b1);
        s.b2 = (float)b2;
        s.w2 = (float)(1.0 - b2);
        s.eps = (float)eps;
        if (RULE == MSM_OPTIM_SGD) {
            s.bc2s = 1.f;
            s.step_size = (float)lr;
        } else {
            const double step = (double)count;
            const double bc1 = 1.0 - pow(b1, step), bc2 = 1.0 - pow(b2, step);
            s.bc2s = (float)sqrt(bc2);
            s.step_size = (float)(lr / bc1);
        }
        s.wd = (float)wd;
        s.lr = (float)lr;
        s.momentum = (float)h[5];
        s.undamped = (float)(1.0 - h[6]);
        s.nesterov = h[7] != 0.0;
        s.first = count <= 1;
        sh = s;
        if (c == 0) {
            float* out = reinterpret_cast<float*>(state + 1);
            out[0] = (float)total;
            out[1] = s.coef;
        }
    }
    __syncthreads();
    const OptScalars s = sh;
    const bool clip = s.coef != 1.f;            // coef == 1 leaves every g as it is
    // g is unscaled in registers right after its load (no multiply without a scale) and written back whenever it changed; the
    // unscaling product is rounded on its own, so a step with a power-of-two scale forms the bits of one without
    const bool unscale = grad_scale != nullptr;
    const bool store_g = unscale || clip;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k.vec) {
        const int n4 = k.n & ~3;
        for (int i = tid * 4; i < n4; i += OPT_T * 4) {
            float4 p = *reinterpret_cast<const float4*>(k.p + i), g = *reinterpret_cast<const float4*>(k.g + i);
            float4 m = use_m ? *reinterpret_cast<const float4*>(k.m + i) : z4;
            float4 v = USE_V ? *reinterpret_cast<const float4*>(k.v + i) : z4;
            opt_rule_update<RULE, OPT_FORM_VEC>(p.x, g.x, m.x, v.x, s, unscale, clip);
            opt_rule_update<RULE, OPT_FORM_VEC>(p.y, g.y, m.y, v.y, s, unscale, clip);
            opt_rule_update<RULE, OPT_FORM_VEC>(p.z, g.z, m.z, v.z, s, unscale, clip);
            opt_rule_update<RULE, OPT_FORM_VEC>(p.w, g.w, m.w, v.w, s, unscale, clip);
            *reinterpret_cast<float4*>(k.p + i) = p;
            if (use_m) *reinterpret_cast<float4*>(k.m + i) = m;
            if (USE_V) *reinterpret_cast<float4*>(k.v + i) = v;
            if (store_g) *reinterpret_cast<float4*>(k.g + i) = g;
        }
        const int i = n4 + tid;
        if (i < k.n) {
            float p = k.p[i], g = k.g[i], m = use_m ? k.m[i] : 0.f, v = USE_V ? k.v[i] : 0.f;
            opt_rule_update<RULE, OPT_FORM_TAIL>(p, g, m, v, s, unscale, clip);
            k.p[i] = p;
            if (use_m) k.m[i] = m;
            if (USE_V) k.v[i] = v;
            if (store_g) k.g[i] = g;
        }
    } else {
        for (int i = tid; i < k.n; i += OPT_T) {
            float p = k.p[i], g = k.g[i], m = use_m ? k.m[i] : 0.f, v = USE_V ? k.v[i] : 0.f;
            opt_rule_update<RULE, OPT_FORM_SCALAR>(p, g, m, v, s, unscale, clip);
            k.p[i] = p;
            if (use_m) k.m[i] = m;
            if (USE_V) k.v[i] = v;
            if (store_g) k.g[i] = g;
        }
    }
}

static bool opt_aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
static bool opt_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace msm

using namespace msm;

extern "C" int msm_optim_chunk(void) { return OPT_CHUNK; }

extern "C" int msm_optim_count_norm(const int64_t* tensors, const int64_t* chunks, double* partials, int64_t* steps, const float* grad_scale,
                                    const float* found_inf, int n_tensors, int n_chunks, int n_rows, void* stream) {
    MSM_REQUIRE(tensors && chunks && partials && steps, "msm_optim_count_norm: null pointer");
    MSM_REQUIRE(opt_aligned8(tensors) && opt_aligned8(chunks) && opt_aligned8(partials) && opt_aligned8(steps),
                "msm_optim_count_norm: the tables, the partials and the step counts must be 8-byte aligned");
    MSM_REQUIRE(opt_aligned4(grad_scale) && opt_aligned4(found_inf), "msm_optim_count_norm: grad_scale and found_inf must be 4-byte aligned");
    MSM_REQUIRE(n_tensors >= 1 && n_chunks >= n_tensors && n_rows >= 1,
                "msm_optim_count_norm: n_tensors = %d, n_chunks = %d, n_rows = %d (every tensor has a chunk and a row)", n_tensors, n_chunks,
                n_rows);
    optim_count_norm_kernel<<<n_chunks, OPT_T, 0, (hipStream_t)stream>>>(tensors, chunks, partials, steps, grad_scale, found_inf, n_tensors,
                                                                        n_rows);
    MSM_CHECK_LAUNCH("msm_optim_count_norm");
    return MSM_OK;
}

extern "C" int msm_optim_update(int rule, const int64_t* tensors, const int64_t* chunks, const double* hyper, const double* partials,
                                int64_t* state, int64_t* steps, const float* grad_scale, const float* found_inf, int n_tensors, int n_chunks,
                                int n_rows, float max_norm, void* stream) {
    MSM_REQUIRE(rule == MSM_OPTIM_ADAMW || rule == MSM_OPTIM_ADAM || rule == MSM_OPTIM_SGD,
                "msm_optim_update: rule = %d (MSM_OPTIM_ADAMW, MSM_OPTIM_ADAM or MSM_OPTIM_SGD)", rule);
    MSM_REQUIRE(tensors && chunks && hyper && state && steps, "msm_optim_update: null pointer");
    MSM_REQUIRE(!(max_norm > 0.f) || partials, "msm_optim_update: max_norm > 0 needs the partials of msm_optim_count_norm");
    MSM_REQUIRE(opt_aligned8(tensors) && opt_aligned8(chunks) && opt_aligned8(hyper) && opt_aligned8(partials) && opt_aligned8(state) &&
                    opt_aligned8(steps),
                "msm_optim_update: the tables, the partials, the state block and the step counts must be 8-byte aligned");
    MSM_REQUIRE(opt_aligned4(grad_scale) && opt_aligned4(found_inf), "msm_optim_update: grad_scale and found_inf must be 4-byte aligned");
    MSM_REQUIRE(n_tensors >= 1 && n_chunks >= n_tensors && n_rows >= 1,
                "msm_optim_update: n_tensors = %d, n_chunks = %d, n_rows = %d (every tensor has a chunk and a row)", n_tensors, n_chunks, n_rows);
    MSM_REQUIRE(max_norm == max_norm, "msm_optim_update: max_norm is nan");
    hipStream_t s = (hipStream_t)stream;
    if (!(max_norm > 0.f)) {
        optim_count_kernel<<<(n_tensors + OPT_T - 1) / OPT_T, OPT_T, 0, s>>>(tensors, steps, found_inf, n_tensors, n_rows);
        MSM_CHECK_LAUNCH("msm_optim_update(counts)");
    }
    if (rule == MSM_OPTIM_ADAMW)
        optim_update_kernel<MSM_OPTIM_ADAMW><<<n_chunks, OPT_T, 0, s>>>(tensors, chunks, hyper, partials, state, steps, grad_scale, found_inf,
                                                                       n_tensors, n_chunks, n_rows, max_norm);
    else if (rule == MSM_OPTIM_ADAM)
        optim_update_kernel<MSM_OPTIM_ADAM><<<n_chunks, OPT_T, 0, s>>>(tensors, chunks, hyper, partials, state, steps, grad_scale, found_inf,
                                                                      n_tensors, n_chunks, n_rows, max_norm);
    else
        optim_update_kernel<MSM_OPTIM_SGD><<<n_chunks, OPT_T, 0, s>>>(tensors, chunks, hyper, partials, state, steps, grad_scale, found_inf,
                                                                     n_tensors, n_chunks, n_rows, max_norm);
    MSM_CHECK_LAUNCH("msm_optim_update");
    return MSM_OK;
}

extern "C" int msm_optim_zero(const int64_t* tensors, const int64_t* chunks, int n_tensors, int n_chunks, void* stream) {
    MSM_REQUIRE(tensors && chunks, "msm_optim_zero: null pointer");
    MSM_REQUIRE(opt_aligned8(tensors) && opt_aligned8(chunks), "msm_optim_zero: the tables must be 8-byte aligned");
    MSM_REQUIRE(n_tensors >= 1 && n_chunks >= n_tensors, "msm_optim_zero: n_tensors = %d, n_chunks = %d (every tensor has a chunk)", n_tensors,
                n_chunks);
    optim_zero_kernel<<<n_chunks, OPT_T, 0, (hipStream_t)stream>>>(tensors, chunks, n_tensors);
    MSM_CHECK_LAUNCH("msm_optim_zero");
    return MSM_OK;
}
