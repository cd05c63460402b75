// Training targets from instance label images (the label half of "raw frames in, loss dict out"): what the reference builds
// on the host per image -- TableTopDataset.__getitem__ lib/datasets/tabletop_dataset.py:319-407 (table -> background,
// process_label_to_annos :183-216, process_label :218-232, sample_pixels :303-316), TabletopDatasetMapper
// lib/datasets/tablet_instance_mapper.py:140-175 and prepare_targets / ImageList.from_tensors
// MSMFormer/meanshiftformer/pretrained_meanshiftformer_model.py:319-321,380-395 -- for a whole batch on the device.
// Every value is an integer or an exact 0 / 1, every counter an integer: the results do not depend on arrival order.
//
//   msm_target_tables   ONE workgroup per image (16 waves) reads the image once, coalesced.  A lane walks its 16-pixel row
//                       segments (1024 segments apart) and keeps the current run (id, count, box) in registers: 16 equal bytes are one vector
//                       compare, any other segment one step per run of equal ids, and only a change of id costs the five
//                       LDS atomics (count, box) -- a few per lane instead of
//                       one set per pixel on a handful of hot addresses.  The ids are ranked with one ballot prefix over
//                       the 1024 bins; the background ids are folded into bin 0 first.
//   msm_target_write    streaming: a lane takes one 16-pixel segment of a padded row, looks its ids up in the image's two
//                       tables (LDS, 4 KiB) once and stores the segment of the label map (64 bytes) and of EVERY mask row of
//                       its image (16 bytes each): a wave writes 1 KiB of contiguous mask row per store instruction, the
//                       label row is read once for all T_b masks.  The rows it may write are the caller's toff clamped to
//                       [0, TT]; a count that disagrees with the device's sets a status bit.
//   msm_sample_labels   sample_pixels as an exact selection: per (image, label) the `num` smallest composites (key, index)
//                       by a radix select -- the pixels per label are counted first (a wave of one label adds once); then
//                       8-bit digits from the top, per digit one histogram launch (LDS-private for the first 32 labels,
//                       integer atomics) and one scan launch that fixes the digit (a wave per label, four bins per lane) --
//                       then one launch that applies the per-label thresholds.  A label is finished as soon as the chosen bin is taken
//                       whole (with random keys after the four key digits), later launches find nothing to do and end.
// Every loop is counted, no workgroup waits on another.
#include "common.h"

namespace {

constexpr int TG_BINS = MSM_TARGET_BINS;
constexpr int TG_MAXI = TG_BINS - 1;                 // instances an image can hold
constexpr int TG_DENSE = 4;                          // table row: 4 header words, ...
constexpr int TG_SLOT = TG_DENSE + TG_BINS;          // ... id -> dense index, id -> mask row, ...
constexpr int TG_INST = TG_SLOT + TG_BINS;           // ... then [TG_MAXI][6] instance records
constexpr int TG_ROW = TG_INST + TG_MAXI * 6;
static_assert(TG_ROW == MSM_TARGET_TABLE_ROW, "msm_hip.h documents the table row");
constexpr int TG_THREADS = 1024;
constexpr int TW_THREADS = 256;

// 16 pixels of one row starting at column xs (nv of them inside the image), as loaded: one 16-byte load (uint8) or four (int32)
// when VEC (whole, aligned segments), element-wise otherwise; get(k) is pixel k as an int
template <typename T, bool VEC>
struct Raw16 {
    int v[16];
    __device__ __forceinline__ void load(const T* __restrict__ row, int xs, int nv) {
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = k < nv ? (int)row[xs + k] : -1;
    }
    __device__ __forceinline__ int get(int k) const { return v[k]; }
};
template <>
struct Raw16<uint8_t, true> {
    uint32_t w[4];
    __device__ __forceinline__ void load(const uint8_t* __restrict__ row, int xs, int) {
        const uint4 q = *reinterpret_cast<const uint4*>(row + xs);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    }
    __device__ __forceinline__ int get(int k) const { return (int)((w[k >> 2] >> (8 * (k & 3))) & 0xffu); }
};
template <>
struct Raw16<int32_t, true> {
    int v[16];
    __device__ __forceinline__ void load(const int32_t* __restrict__ row, int xs, int) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int4 q = *reinterpret_cast<const int4*>(row + xs + 4 * j);
            v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
        }
    }
    __device__ __forceinline__ int get(int k) const { return v[k]; }
};

template <typename T, bool VEC>
__device__ __forceinline__ void load16(const T* __restrict__ row, int xs, int nv, int (&v)[16]) {
    Raw16<T, VEC> r;
    r.load(row, xs, nv);
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = r.get(k);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(TG_THREADS) void target_tables_kernel(const T* __restrict__ raw, const int32_t* __restrict__ bg, int n_bg,
                                                                   int32_t* __restrict__ tables, int H, int W) {
    __shared__ int cnt[TG_BINS], xmn[TG_BINS], ymn[TG_BINS], xmx[TG_BINS], ymx[TG_BINS];
    __shared__ int wsum[TG_THREADS / 64];
    __shared__ int bad_s;
    const int b = blockIdx.x, tid = threadIdx.x;
    cnt[tid] = 0; xmn[tid] = W; ymn[tid] = H; xmx[tid] = -1; ymx[tid] = -1;
    if (tid == 0) bad_s = 0;
    __syncthreads();
    const T* img = raw + (int64_t)b * H * W;
    const int segs = (W + 15) / 16, units = H * segs;
    const int per = (units + TG_THREADS - 1) / TG_THREADS;       // segments per lane: lane t takes t, t + 1024, ... (coalesced)
    int cur = -1, n = 0, x0 = 0, x1 = 0, y0 = 0, y1 = 0, bad = 0;
    auto flush = [&]() {
        if (n > 0) {
            atomicAdd(&cnt[cur], n);
            atomicMin(&xmn[cur], x0); atomicMax(&xmx[cur], x1);
            atomicMin(&ymn[cur], y0); atomicMax(&ymx[cur], y1);
        }
    };
    // NB segments are loaded before the first is looked at: the lane's walk is a chain of dependent steps, the loads are not.
    // A run needs equal ids, not neighbours: the segments of a lane lie rows apart and still merge wherever the image is uniform.
    constexpr int NB = sizeof(Raw16<T, VEC>) <= 16 ? 8 : 2;
    for (int ib = 0; ib < per; ib += NB) {
        Raw16<T, VEC> seg[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int64_t uu = (int64_t)(ib + j) * TG_THREADS + tid;
            const int u = (int)(uu < units ? uu : units - 1);
            const int y = u / segs, xs = (u - y * segs) * 16;
            seg[j].load(img + (int64_t)y * W, xs, W - xs < 16 ? W - xs : 16);
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int64_t uu = (int64_t)(ib + j) * TG_THREADS + tid;
            if (ib + j >= per || uu >= units) continue;
            const int u = (int)uu;
            const int y = u / segs, xs = (u - y * segs) * 16;
            const int nv = W - xs < 16 ? W - xs : 16;
            bool same = nv == 16 && cur >= 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) same = same && seg[j].get(k) == cur;
            if (same) {                                    // the run goes on over the whole segment
                n += 16;
                x0 = x0 < xs ? x0 : xs; x1 = x1 > xs + 15 ? x1 : xs + 15; y1 = y;
                continue;
            }
            unsigned starts = 1u;                          // bit k: a run of equal ids starts at pixel k of the segment
#pragma unroll
            for (int k = 1; k < 16; ++k) starts |= (k < nv && seg[j].get(k) != seg[j].get(k - 1)) ? (1u << k) : 0u;
            for (int r = 0; r < 16 && starts; ++r) {       // one step per run (two at an object edge), not per pixel
                const int a = __ffs((int)starts) - 1;
                starts &= starts - 1u;
                const int e = starts ? __ffs((int)starts) - 1 : nv;
                int id = seg[j].get(0);
#pragma unroll
                for (int k = 1; k < 16; ++k) id = a == k ? seg[j].get(k) : id;
                const int len = e - a, xa = xs + a, xb = xs + e - 1;
                if ((unsigned)id >= (unsigned)TG_BINS) { bad += len; continue; }
                if (id == cur) {
                    n += len;
                    x0 = x0 < xa ? x0 : xa; x1 = x1 > xb ? x1 : xb; y1 = y;
                } else {
                    flush();
                    cur = id; n = len; x0 = xa; x1 = xb; y0 = y1 = y;
                }
            }
        }
    }
    flush();
    if (bad) atomicAdd(&bad_s, bad);
    bool isbg = false;                                     // fold: the background ids count as id 0 (they never are instances)
    for (int i = 0; i < n_bg; ++i) isbg = isbg || bg[i] == tid;
    isbg = isbg && tid > 0;
    __syncthreads();
    if (isbg && cnt[tid] > 0) atomicAdd(&cnt[0], cnt[tid]);
    __syncthreads();
    if (isbg) cnt[tid] = 0;
    __syncthreads();
    const int p = cnt[tid] > 0 ? 1 : 0;                    // rank of the present values: the dense index
    const unsigned long long bal = __ballot(p);
    const int lane = tid & 63, w = tid >> 6;
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int base = 0, K = 0;
#pragma unroll
    for (int i = 0; i < TG_THREADS / 64; ++i) {
        base += i < w ? wsum[i] : 0;
        K += wsum[i];
    }
    const int r = base + __popcll(bal & ((1ull << lane) - 1ull));
    const int p0 = cnt[0] > 0 ? 1 : 0;
    const int Tb = K - p0;
    int32_t* tab = tables + (int64_t)b * TG_ROW;
    // without a background pixel the lowest id takes dense index 0 and still is instance 0 (process_label does the same)
    const int slot = (p && tid > 0) ? r - p0 : -1;
    tab[TG_DENSE + tid] = isbg ? (p0 ? 0 : -1) : (p ? r : -1);
    tab[TG_SLOT + tid] = slot;
    if (slot >= 0) {
        int32_t* rec = tab + TG_INST + slot * 6;
        rec[0] = tid; rec[1] = cnt[tid]; rec[2] = xmn[tid]; rec[3] = ymn[tid]; rec[4] = xmx[tid]; rec[5] = ymx[tid];
    }
    for (int i = Tb * 6 + tid; i < TG_MAXI * 6; i += TG_THREADS) tab[TG_INST + i] = 0;
    if (tid == 0) { tab[0] = bad_s; tab[1] = Tb; tab[2] = K; tab[3] = 0; }
}

template <typename T, bool VIN, bool VOUT>
__global__ __launch_bounds__(TW_THREADS) void target_write_kernel(const T* __restrict__ raw, int32_t* __restrict__ tables,
                                                                  const int64_t* __restrict__ toff, int32_t* __restrict__ label_out,
                                                                  uint8_t* __restrict__ masks, float* __restrict__ boxes,
                                                                  int32_t* __restrict__ ids, int32_t* __restrict__ areas, int H, int W,
                                                                  int Hp, int Wp, int64_t TT, int label_float) {
    __shared__ short s_dense[TG_BINS], s_slot[TG_BINS];
    const int b = blockIdx.y, tid = threadIdx.x;
    int32_t* tab = tables + (int64_t)b * TG_ROW;
    const int segs = (Wp + 15) / 16, units = Hp * segs;
    const T* img = raw + (int64_t)b * H * W;
    int v[16];                                             // the lane's first segment, requested ahead of the table staging
    const int ufirst = blockIdx.x * TW_THREADS + tid;
    {
        const int y = ufirst / segs, xs = (ufirst - y * segs) * 16;
        if (ufirst < units && y < H && xs < W) load16<T, VIN>(img + (int64_t)y * W, xs, W - xs < 16 ? W - xs : 16, v);
    }
    for (int i = tid; i < TG_BINS; i += TW_THREADS) {
        s_dense[i] = (short)tab[TG_DENSE + i];
        s_slot[i] = (short)tab[TG_SLOT + i];
    }
    const int Tb = tab[1];
    int64_t r0 = 0;
    int nrows = 0;
    if (masks != nullptr) {                                // the rows this image may write: the caller's, clamped into the buffer
        int64_t a = toff[b], e = toff[b + 1];
        a = a < 0 ? 0 : (a > TT ? TT : a);
        e = e < a ? a : (e > TT ? TT : e);
        r0 = a;
        nrows = (int)(e - a < (int64_t)TG_BINS ? e - a : (int64_t)TG_BINS);
        if (blockIdx.x == 0) {
            if (tid == 0 && (toff[b + 1] - toff[b] != (int64_t)Tb || e - a != (int64_t)Tb)) atomicOr(&tab[3], 1);
            for (int64_t t = tid; t < e - a; t += TW_THREADS) {                // the compact per-instance rows
                const bool have = t < Tb;
                const int32_t* rec = tab + TG_INST + (have ? (int)t : 0) * 6;
                ids[a + t] = have ? rec[0] : 0;
                areas[a + t] = have ? rec[1] : 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) boxes[(a + t) * 4 + j] = have ? (float)rec[2 + j] : 0.f;
            }
        }
    }
    __syncthreads();
    const int64_t plane = (int64_t)Hp * Wp;
    for (int u = ufirst; u < units; u += gridDim.x * TW_THREADS) {
        const int y = u / segs, xs = (u - y * segs) * 16;
        int dn[16], sl[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) { dn[k] = 0; sl[k] = -1; }
        if (y < H && xs < W) {
            const int nv = W - xs < 16 ? W - xs : 16;
            if (u != ufirst) load16<T, VIN>(img + (int64_t)y * W, xs, nv, v);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (k < nv && (unsigned)v[k] < (unsigned)TG_BINS) {            // a pixel outside [0, 1024) is written as background
                    const int d = s_dense[v[k]];
                    dn[k] = d < 0 ? 0 : d;
                    sl[k] = s_slot[v[k]];
                }
            }
        }
        const int64_t o = (int64_t)y * Wp + xs;
        int32_t* lrow = label_out + (int64_t)b * plane + o;
#pragma unroll
        for (int k = 0; k < 16; ++k) dn[k] = label_float ? __float_as_int((float)dn[k]) : dn[k];
        if (VOUT) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<int4*>(lrow + 4 * j) = make_int4(dn[4 * j], dn[4 * j + 1], dn[4 * j + 2], dn[4 * j + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (xs + k < Wp) lrow[k] = dn[k];
        }
        for (int t = 0; t < nrows; ++t) {                  // rows from T_b on (a caller's count too large) become zero rows
            uint32_t wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 16; ++k) wd[k >> 2] |= (sl[k] == t ? 1u : 0u) << (8 * (k & 3));
            uint8_t* mrow = masks + (r0 + t) * plane + o;
            if (VOUT) {
                *reinterpret_cast<uint4*>(mrow) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (xs + k < Wp) mrow[k] = (uint8_t)((wd[k >> 2] >> (8 * (k & 3))) & 1u);
            }
        }
    }
}

// ---- sample_pixels -------------------------------------------------------------------------------------------------------
constexpr int SP_LABELS = MSM_SAMPLE_MAX_LABELS;       // dense labels per image
constexpr int SP_LDS_LABELS = 32;                      // labels whose histogram a workgroup keeps in LDS
constexpr int SP_THREADS = 512;
constexpr int SP_CHUNK = 16384;                        // pixels per workgroup of the histogram / apply launches

// workspace of one image: prefix / threshold, rank still wanted, mode (0 keep all, 1 selecting, 2 threshold known), count, histogram
struct SampleState {
    unsigned long long prefix[SP_LABELS];
    int32_t k[SP_LABELS];
    int32_t mode[SP_LABELS];
    int32_t n[SP_LABELS];
    int32_t pad[SP_LABELS];
    int32_t hist[SP_LABELS][256];
};
static_assert(sizeof(SampleState) % 16 == 0, "the histogram is cleared with 16-byte stores");

// the dense label of a pixel: -1 = ignored, -2 = not an integer in [0, 256)
__device__ __forceinline__ int label_of(const int32_t* __restrict__ labels, int64_t at, int label_float) {
    const int32_t w = labels[at];
    if (!label_float) return w < 0 ? -1 : (w < SP_LABELS ? w : -2);
    const float f = __int_as_float(w);
    if (f < 0.f) return -1;
    if (!(f < (float)SP_LABELS)) return -2;
    const int l = (int)f;
    return (float)l == f ? l : -2;
}

// (key, index) as one left-aligned unsigned number of 8 * passes bits: signed key order, ties to the lower index
__device__ __forceinline__ unsigned long long composite(int32_t key, uint32_t idx, int index_bits, int align) {
    return ((((unsigned long long)((uint32_t)key ^ 0x80000000u)) << index_bits) | idx) << align;
}

// clear: the state of every label (mode 3 = not counted yet), the histogram, the status word
__global__ __launch_bounds__(TG_THREADS) void sample_clear_kernel(SampleState* __restrict__ ws, int32_t* __restrict__ status, int num) {
    SampleState* st = ws + blockIdx.x;
    const int tid = threadIdx.x;
    if (tid < SP_LABELS) {
        st->prefix[tid] = 0ull;
        st->k[tid] = num;
        st->mode[tid] = 3;
        st->n[tid] = 0;
        st->pad[tid] = 0;
    }
    int4* h = reinterpret_cast<int4*>(&st->hist[0][0]);
    for (int i = tid; i < SP_LABELS * 256 / 4; i += TG_THREADS) h[i] = make_int4(0, 0, 0, 0);
    if (tid == 0) status[blockIdx.x] = 0;
}

// count: pixels per label.  A wave whose 64 pixels carry one label (the usual case inside an object) adds once.
__global__ __launch_bounds__(SP_THREADS) void sample_count_kernel(const int32_t* __restrict__ labels, SampleState* __restrict__ ws,
                                                                  int32_t* __restrict__ status, int H, int W, int Hp, int Wp,
                                                                  int label_float) {
    __shared__ int s_n[SP_LABELS];
    __shared__ int bad_s;
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid < SP_LABELS) s_n[tid] = 0;
    if (tid == 0) bad_s = 0;
    __syncthreads();
    const int total = H * W;
    const int p_end = (blockIdx.x + 1) * SP_CHUNK < total ? (blockIdx.x + 1) * SP_CHUNK : total;
    const int64_t base = (int64_t)b * Hp * Wp;
    int bad = 0;
    for (int p0 = blockIdx.x * SP_CHUNK; p0 < p_end; p0 += SP_THREADS) {       // uniform trip count: the ballots see whole waves
        const int p = p0 + tid;
        int l = -1;
        if (p < p_end) {
            const int y = p / W, x = p - y * W;
            l = label_of(labels, base + (int64_t)y * Wp + x, label_float);
        }
        if (l == -2) ++bad;
        const int first = __builtin_amdgcn_readfirstlane(l);
        if (__all(l == first)) {
            if ((tid & 63) == 0 && first >= 0) atomicAdd(&s_n[first], 64);
        } else if (l >= 0) {
            atomicAdd(&s_n[l], 1);
        }
    }
    if (bad) atomicAdd(&bad_s, bad);
    __syncthreads();
    if (tid < SP_LABELS && s_n[tid]) atomicAdd(&ws[b].n[tid], s_n[tid]);
    if (tid == 0 && bad_s) atomicAdd(&status[b], bad_s);
}

__global__ __launch_bounds__(SP_THREADS) void sample_hist_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ keys,
                                                                 SampleState* __restrict__ ws, int H, int W, int Hp, int Wp, int shift,
                                                                 int index_bits, int align, int label_float, int num) {
    __shared__ unsigned long long s_prefix[SP_LABELS];
    __shared__ int s_mode[SP_LABELS];
    __shared__ int s_hist[SP_LDS_LABELS * 256];
    const int b = blockIdx.y, tid = threadIdx.x;
    SampleState* st = ws + b;
    int active = 0;
    if (tid < SP_LABELS) {
        const int mode = st->mode[tid];
        s_mode[tid] = mode == 3 ? (st->n[tid] > num ? 1 : 0) : mode;       // first digit: the counts decide who selects
        s_prefix[tid] = st->prefix[tid];
        active = s_mode[tid] == 1;
    }
    for (int i = tid; i < SP_LDS_LABELS * 256; i += SP_THREADS) s_hist[i] = 0;
    if (!__syncthreads_or(active)) return;                 // every label of this image is settled
    const int total = H * W;
    const int p_end = (blockIdx.x + 1) * SP_CHUNK < total ? (blockIdx.x + 1) * SP_CHUNK : total;
    const int64_t base = (int64_t)b * Hp * Wp;
    for (int p = blockIdx.x * SP_CHUNK + tid; p < p_end; p += SP_THREADS) {
        const int y = p / W, x = p - y * W;
        const int l = label_of(labels, base + (int64_t)y * Wp + x, label_float);
        if (l < 0 || s_mode[l] != 1) continue;
        const unsigned long long c = composite(keys[(int64_t)b * total + p], (uint32_t)p, index_bits, align);
        if ((c >> (shift + 8)) != s_prefix[l]) continue;
        const int d = (int)((c >> shift) & 0xffull);
        if (l < SP_LDS_LABELS) atomicAdd(&s_hist[l * 256 + d], 1);
        else atomicAdd(&st->hist[l][d], 1);
    }
    __syncthreads();
    for (int i = tid; i < SP_LDS_LABELS * 256; i += SP_THREADS) {
        const int c = s_hist[i];
        if (c) atomicAdd(&st->hist[0][0] + i, c);
    }
}

// scan: one wave per (image, label); a lane holds four bins, the running sum is a wave scan
__global__ __launch_bounds__(256) void sample_scan_kernel(SampleState* __restrict__ ws, int shift, int num) {
    SampleState* st = ws + blockIdx.y;
    const int lane = threadIdx.x & 63, l = blockIdx.x * 4 + (threadIdx.x >> 6);
    int mode = st->mode[l];
    if (mode == 3) {                                       // first digit: settle the labels that keep everything
        mode = st->n[l] > num ? 1 : 0;
        if (mode == 0 && lane == 0) st->mode[l] = 0;
    }
    if (mode != 1) return;
    int4* h = reinterpret_cast<int4*>(&st->hist[l][0]);
    const int4 q = h[lane];
    h[lane] = make_int4(0, 0, 0, 0);
    const int c[4] = {q.x, q.y, q.z, q.w};
    const int mine = c[0] + c[1] + c[2] + c[3];
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    int k = st->k[l];
    const unsigned long long reached = __ballot(incl >= k);
    const int sel = reached ? __ffsll((long long)reached) - 1 : 63;
    if (lane != sel) return;
    int cum = incl - mine, digit = 255, in_bin = 0;
    bool found = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!found && cum + c[j] >= k) { found = true; digit = 4 * lane + j; in_bin = c[j]; k -= cum; }
        cum += c[j];
    }
    const unsigned long long prefix = (st->prefix[l] << 8) | (unsigned long long)digit;
    if (!found || in_bin == k || shift == 0) {             // the bin is taken whole (or this was the last digit): the threshold
        st->prefix[l] = (prefix << shift) | ((1ull << shift) - 1ull);
        st->mode[l] = 2;
    } else {
        st->prefix[l] = prefix;
        st->k[l] = k;
        st->mode[l] = 1;
    }
}

__global__ __launch_bounds__(SP_THREADS) void sample_apply_kernel(int32_t* __restrict__ labels, const int32_t* __restrict__ keys,
                                                                  const SampleState* __restrict__ ws, int H, int W, int Hp, int Wp,
                                                                  int index_bits, int align, int label_float) {
    __shared__ unsigned long long s_thresh[SP_LABELS];
    __shared__ int s_mode[SP_LABELS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const SampleState* st = ws + b;
    int active = 0;
    if (tid < SP_LABELS) {
        s_mode[tid] = st->mode[tid];
        s_thresh[tid] = st->prefix[tid];
        active = s_mode[tid] != 0;
    }
    if (!__syncthreads_or(active)) return;                 // no label of this image has more than num pixels
    const int total = H * W;
    const int p_end = (blockIdx.x + 1) * SP_CHUNK < total ? (blockIdx.x + 1) * SP_CHUNK : total;
    const int64_t base = (int64_t)b * Hp * Wp;
    const int32_t ignore = label_float ? __float_as_int(-1.f) : -1;
    for (int p = blockIdx.x * SP_CHUNK + tid; p < p_end; p += SP_THREADS) {
        const int y = p / W, x = p - y * W;
        const int64_t at = base + (int64_t)y * Wp + x;
        const int l = label_of(labels, at, label_float);
        if (l < 0 || s_mode[l] == 0) continue;
        const unsigned long long c = composite(keys[(int64_t)b * total + p], (uint32_t)p, index_bits, align);
        if (c > s_thresh[l]) labels[at] = ignore;
    }
}

template <typename T>
int launch_tables(const T* raw, const int32_t* bg, int n_bg, int32_t* tables, int B, int H, int W, hipStream_t s) {
    const bool vec = W % 16 == 0 && ((uintptr_t)raw & 15) == 0;
    if (vec) hipLaunchKernelGGL((target_tables_kernel<T, true>), dim3(B), dim3(TG_THREADS), 0, s, raw, bg, n_bg, tables, H, W);
    else hipLaunchKernelGGL((target_tables_kernel<T, false>), dim3(B), dim3(TG_THREADS), 0, s, raw, bg, n_bg, tables, H, W);
    return 0;
}

template <typename T>
void launch_write(dim3 grid, hipStream_t s, bool vin, bool vout, const T* raw, int32_t* tables, const int64_t* toff, int32_t* label_out,
                  uint8_t* masks, float* boxes, int32_t* ids, int32_t* areas, int H, int W, int Hp, int Wp, int64_t TT, int label_float) {
#define MSM_TW(VI, VO)                                                                                                              \
    hipLaunchKernelGGL((target_write_kernel<T, VI, VO>), grid, dim3(TW_THREADS), 0, s, raw, tables, toff, label_out, masks, boxes, ids, \
                       areas, H, W, Hp, Wp, TT, label_float)
    if (vin && vout) MSM_TW(true, true);
    else if (vin) MSM_TW(true, false);
    else if (vout) MSM_TW(false, true);
    else MSM_TW(false, false);
#undef MSM_TW
}

bool image_shape_ok(int B, int H, int W) {
    return B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 24);
}

}  // namespace

extern "C" int msm_target_table_row(void) { return TG_ROW; }

extern "C" int msm_target_tables(const void* raw, int raw_is_i32, const int32_t* background_ids, int n_background, int32_t* tables,
                                 int B, int H, int W, void* stream) {
    MSM_REQUIRE(raw && tables, "msm_target_tables: null pointer");
    MSM_REQUIRE(image_shape_ok(B, H, W), "msm_target_tables: bad shape B=%d H=%d W=%d (B <= 65535, H W <= 2^24)", B, H, W);
    MSM_REQUIRE(n_background >= 0 && n_background <= 16 && (n_background == 0 || background_ids),
                "msm_target_tables: 0..16 background ids");
    MSM_REQUIRE(((uintptr_t)tables & 3) == 0 && ((uintptr_t)background_ids & 3) == 0 && (!raw_is_i32 || ((uintptr_t)raw & 3) == 0),
                "msm_target_tables: misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    if (raw_is_i32) launch_tables(static_cast<const int32_t*>(raw), background_ids, n_background, tables, B, H, W, s);
    else launch_tables(static_cast<const uint8_t*>(raw), background_ids, n_background, tables, B, H, W, s);
    MSM_CHECK_LAUNCH("msm_target_tables");
    return MSM_OK;
}

extern "C" int msm_target_write(const void* raw, int raw_is_i32, int32_t* tables, const int64_t* toff, void* label_out, int label_is_f32,
                                uint8_t* masks, float* boxes, int32_t* ids, int32_t* areas, int B, int H, int W, int Hp, int Wp,
                                int64_t TT, void* stream) {
    MSM_REQUIRE(raw && tables && label_out, "msm_target_write: null pointer (raw, tables and label_out are required)");
    MSM_REQUIRE(image_shape_ok(B, H, W), "msm_target_write: bad shape B=%d H=%d W=%d (B <= 65535, H W <= 2^24)", B, H, W);
    MSM_REQUIRE(Hp >= H && Wp >= W && (int64_t)Hp * Wp <= ((int64_t)1 << 26),
                "msm_target_write: the frame %dx%d must hold the image %dx%d (and at most 2^26 pixels)", Hp, Wp, H, W);
    MSM_REQUIRE(masks == nullptr || (toff && boxes && ids && areas && TT >= 0),
                "msm_target_write: masks need toff, boxes, ids and areas");
    MSM_REQUIRE((((uintptr_t)tables | (uintptr_t)label_out | (uintptr_t)boxes | (uintptr_t)ids | (uintptr_t)areas) & 3) == 0 &&
                    ((uintptr_t)toff & 7) == 0 && (!raw_is_i32 || ((uintptr_t)raw & 3) == 0),
                "msm_target_write: misaligned pointer");
    const bool vin = W % 16 == 0 && ((uintptr_t)raw & 15) == 0;
    const bool vout = Wp % 16 == 0 && (((uintptr_t)label_out | (uintptr_t)masks) & 15) == 0;
    const int units = Hp * ((Wp + 15) / 16);
    const dim3 grid((unsigned)max(1, min(msm::cdiv(units, TW_THREADS), 2048)), (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    if (raw_is_i32)
        launch_write(grid, s, vin, vout, static_cast<const int32_t*>(raw), tables, toff, static_cast<int32_t*>(label_out), masks, boxes,
                     ids, areas, H, W, Hp, Wp, TT, label_is_f32 ? 1 : 0);
    else
        launch_write(grid, s, vin, vout, static_cast<const uint8_t*>(raw), tables, toff, static_cast<int32_t*>(label_out), masks, boxes,
                     ids, areas, H, W, Hp, Wp, TT, label_is_f32 ? 1 : 0);
    MSM_CHECK_LAUNCH("msm_target_write");
    return MSM_OK;
}

extern "C" int64_t msm_sample_labels_workspace(int B) {
    if (B <= 0 || B > 65535) {
        msm::set_error("msm_sample_labels_workspace: bad batch %d", B);
        return MSM_E_INVALID;
    }
    return (int64_t)B * (int64_t)sizeof(SampleState);
}

extern "C" int msm_sample_labels(void* labels, int label_is_f32, const int32_t* keys, int32_t* status, void* workspace,
                                 int64_t workspace_bytes, int B, int H, int W, int Hp, int Wp, int num, void* stream) {
    MSM_REQUIRE(labels && keys && status && workspace, "msm_sample_labels: null pointer");
    MSM_REQUIRE(image_shape_ok(B, H, W), "msm_sample_labels: bad shape B=%d H=%d W=%d (B <= 65535, H W <= 2^24)", B, H, W);
    MSM_REQUIRE(Hp >= H && Wp >= W && (int64_t)Hp * Wp <= ((int64_t)1 << 26),
                "msm_sample_labels: the frame %dx%d must hold the image %dx%d (and at most 2^26 pixels)", Hp, Wp, H, W);
    MSM_REQUIRE(num >= 1, "msm_sample_labels: num must be at least 1, got %d", num);
    MSM_REQUIRE((((uintptr_t)labels | (uintptr_t)keys | (uintptr_t)status) & 3) == 0 && ((uintptr_t)workspace & 15) == 0,
                "msm_sample_labels: misaligned pointer");
    if (workspace_bytes < (int64_t)B * (int64_t)sizeof(SampleState)) {
        msm::set_error("msm_sample_labels: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                       (long long)((int64_t)B * (int64_t)sizeof(SampleState)));
        return MSM_E_WORKSPACE;
    }
    int index_bits = 1;
    while (((int64_t)1 << index_bits) < (int64_t)H * W) ++index_bits;
    const int passes = (32 + index_bits + 7) / 8, align = 8 * passes - (32 + index_bits);      // at most 7 digits
    hipStream_t s = (hipStream_t)stream;
    int32_t* lab = static_cast<int32_t*>(labels);
    SampleState* ws = static_cast<SampleState*>(workspace);
    const int lf = label_is_f32 ? 1 : 0;
    const dim3 grid((unsigned)msm::cdiv((int64_t)H * W, SP_CHUNK), (unsigned)B);
    hipLaunchKernelGGL(sample_clear_kernel, dim3(B), dim3(TG_THREADS), 0, s, ws, status, num);
    hipLaunchKernelGGL(sample_count_kernel, grid, dim3(SP_THREADS), 0, s, lab, ws, status, H, W, Hp, Wp, lf);
    for (int pass = 0; pass < passes; ++pass) {
        const int shift = 8 * (passes - 1 - pass);
        hipLaunchKernelGGL(sample_hist_kernel, grid, dim3(SP_THREADS), 0, s, lab, keys, ws, H, W, Hp, Wp, shift, index_bits, align, lf, num);
        hipLaunchKernelGGL(sample_scan_kernel, dim3(SP_LABELS / 4, B), dim3(256), 0, s, ws, shift, num);
    }
    hipLaunchKernelGGL(sample_apply_kernel, grid, dim3(SP_THREADS), 0, s, lab, keys, ws, H, W, Hp, Wp, index_bits, align, lf);
    MSM_CHECK_LAUNCH("msm_sample_labels");
    return MSM_OK;
}
