// densify.hip — adaptive density control (include/dvs_train.h), HBM-streaming kernels:
// statistics accumulation, plan (action + exclusive scan of output counts) and apply (scatter of parameters / optimizer moments).
#include <hip/hip_runtime.h>
#include "../../include/dvs_train.h"
#include "../../include/dvs_raster.h"
#include "dvs_device.h"
#include "block_scan.h"

__device__ __forceinline__ float d_normal(uint32_t seed, uint32_t id, uint32_t k) {
    const float u1 = dvs_uniform24(dvs_hash3(seed, id, 2 * k)), u2 = dvs_uniform24(dvs_hash3(seed, id, 2 * k + 1));
    return sqrtf(-2.0f * __logf(u1)) * __cosf(6.2831853f * u2);
}

__global__ void __launch_bounds__(DB)
k_densify_accumulate(int n, const int* __restrict__ radii, const float2* __restrict__ absgrad, float half_w, float half_h,
                     float* __restrict__ grad_accum, float* __restrict__ denom, int* __restrict__ max_radii) {
    const int i = blockIdx.x * DB + threadIdx.x;
    if (i >= n) return;
    const int r = radii[i];
    if (r <= 0) return;
    const float2 g = absgrad[i];
    const float gx = g.x * half_w, gy = g.y * half_h;
    grad_accum[i] += sqrtf(gx * gx + gy * gy);
    denom[i] += 1.0f;
    max_radii[i] = max(max_radii[i], r);
}

// the same rule for the n_views views of a multi-view pass, read from the composite backward's rows BEFORE the preprocess backward
// consumes them (row floats 9, 10 = sum over the view's pixels of |dL/dmean2D| x, y: exactly what A9 hands out as absgrad2d)
__global__ void __launch_bounds__(DB)
k_densify_accumulate_rows(int n, int n_views, const int* __restrict__ radii, const float* __restrict__ rows, float half_w, float half_h,
                          float* __restrict__ grad_accum, float* __restrict__ denom, int* __restrict__ max_radii) {
    const int i = blockIdx.x * DB + threadIdx.x;
    if (i >= n) return;
    float acc = 0.f, cnt = 0.f;
    int rmax = 0;
    for (int v = 0; v < n_views; ++v) {
        const int r = radii[(size_t)v * n + i];
        if (r <= 0) continue;
        const float* row = rows + ((size_t)v * n + i) * 12;
        const float gx = row[9] * half_w, gy = row[10] * half_h;
        acc += sqrtf(gx * gx + gy * gy);
        cnt += 1.0f;
        rmax = max(rmax, r);
    }
    if (cnt > 0.f) {
        grad_accum[i] += acc;
        denom[i] += cnt;
        max_radii[i] = max(max_radii[i], rmax);
    }
}
// radius > 0 in any of the views (visibleAdam with several views per step)
__global__ void __launch_bounds__(DB) k_any_view_radius(int n, int n_views, const int* __restrict__ radii, int* __restrict__ out) {
    const int i = blockIdx.x * DB + threadIdx.x;
    if (i >= n) return;
    int r = 0;
    for (int v = 0; v < n_views; ++v) r = max(r, radii[(size_t)v * n + i]);
    out[i] = r;
}

__device__ __forceinline__ int d_action(int i, const float* opacity, const float* scale, const float* grad_accum, const float* denom,
                                        const int* max_radii, const dvs_densify_params& p) {
    const float lo = opacity[i], s0 = scale[3 * (int64_t)i], s1 = scale[3 * (int64_t)i + 1], s2 = scale[3 * (int64_t)i + 2];
    // a splat with a non-finite opacity or scale is culled by every forward and would otherwise be KEEP for ever (NaN fails `<`,
    // fmaxf drops a NaN scale, an infinite one never gathers statistics): it goes, whatever the limits and the cap
    if (!(isfinite(lo) && isfinite(s0) && isfinite(s1) && isfinite(s2))) return DVS_DENSIFY_PRUNE;
    const float op = 1.0f / (1.0f + __expf(-lo));
    const float smax = __expf(fmaxf(s0, fmaxf(s1, s2)));
    if (op < p.min_opacity) return DVS_DENSIFY_PRUNE;
    if (p.max_world_scale > 0.f && smax > p.max_world_scale) return DVS_DENSIFY_PRUNE;
    if (p.max_screen_radius > 0 && max_radii[i] > p.max_screen_radius) return DVS_DENSIFY_PRUNE;
    const float d = denom[i];
    const float avg = d > 0.f ? grad_accum[i] / d : 0.f;
    if (!(avg >= p.grad_threshold)) return DVS_DENSIFY_KEEP;
    return smax > p.scale_threshold ? DVS_DENSIFY_SPLIT : DVS_DENSIFY_CLONE;
}
__device__ __forceinline__ bool d_grows(int a) { return a == DVS_DENSIFY_CLONE || a == DVS_DENSIFY_SPLIT; }

// per block: (surviving splats) | (growth candidates << 16), both <= DB
__global__ void __launch_bounds__(DB)
k_densify_blocksum(int n, const float* __restrict__ opacity, const float* __restrict__ scale, const float* __restrict__ grad_accum,
                   const float* __restrict__ denom, const int* __restrict__ max_radii, dvs_densify_params p, uint8_t* __restrict__ action,
                   uint32_t* __restrict__ block_sums) {
    __shared__ uint32_t tmp[DB / 64];
    const int i = blockIdx.x * DB + threadIdx.x;
    int a = DVS_DENSIFY_PRUNE;
    if (i < n) { a = d_action(i, opacity, scale, grad_accum, denom, max_radii, p); action[i] = (uint8_t)a; }
    uint32_t tot;
    (void)dvs_block_excl_scan((a != DVS_DENSIFY_PRUNE ? 1u : 0u) | (d_grows(a) ? 1u << 16 : 0u), tmp, &tot);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}
// single workgroup over the nb packed block sums, DB blocks per chunk with a running carry. Pass 1: totals S (survivors) and G (growth
// candidates); the growth budget is G, or min(G, cap_max - S) (>= 0) when cap_max > 0, and the new count is S + budget. Pass 2: block
// offsets = survivors before the block + accepted growth before it, where growth is accepted in splat order until the budget is spent.
// The one block in which the budget runs out ("cut" block) and what is left of the budget there (< its candidates, so < DB) go to the
// word after the block offsets: block_sums[nb] = cut << 8 | left (cut = nb: every candidate is accepted).
__global__ void __launch_bounds__(DB)
k_densify_scan_blocks(uint32_t* __restrict__ block_sums, uint32_t nb, int cap_max, uint64_t* __restrict__ total) {
    __shared__ uint32_t tmp[DB / 64];
    __shared__ uint32_t cut_word;
    uint64_t S = 0, G = 0;
    for (uint32_t base = 0; base < nb; base += DB) {
        const uint32_t idx = base + threadIdx.x;
        const uint32_t v = idx < nb ? block_sums[idx] : 0u;
        uint32_t ts, tg;
        (void)dvs_block_excl_scan(v & 0xffffu, tmp, &ts);
        (void)dvs_block_excl_scan(v >> 16, tmp, &tg);
        S += ts; G += tg;
    }
    const uint64_t budget = cap_max > 0 ? ((uint64_t)cap_max > S ? min(G, (uint64_t)cap_max - S) : 0ull) : G;
    if (threadIdx.x == 0) cut_word = nb << 8;
    __syncthreads();
    uint64_t cs = 0, cg = 0;
    for (uint32_t base = 0; base < nb; base += DB) {
        const uint32_t idx = base + threadIdx.x;
        const uint32_t v = idx < nb ? block_sums[idx] : 0u;
        uint32_t ts, tg;
        const uint64_t es = cs + dvs_block_excl_scan(v & 0xffffu, tmp, &ts);
        const uint64_t eg = cg + dvs_block_excl_scan(v >> 16, tmp, &tg);
        if (idx < nb) {
            block_sums[idx] = (uint32_t)(es + min(eg, budget));
            if (eg <= budget && budget < eg + (v >> 16)) cut_word = idx << 8 | (uint32_t)(budget - eg);     // (one block at most)
        }
        cs += ts; cg += tg;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *total = S + budget;
        if (nb) block_sums[nb] = cut_word;
    }
}
// growth candidates past the budget are demoted to KEEP (action rewritten); offsets = exclusive scan of the final output counts
__global__ void __launch_bounds__(DB)
k_densify_offsets(int n, uint8_t* __restrict__ action, const uint32_t* __restrict__ block_offsets, uint32_t* __restrict__ offsets) {
    __shared__ uint32_t tmp[DB / 64];
    const int i = blockIdx.x * DB + threadIdx.x;
    int a = i < n ? action[i] : DVS_DENSIFY_PRUNE;
    const uint32_t cut = block_offsets[gridDim.x];
    const uint32_t quota = blockIdx.x < (cut >> 8) ? (uint32_t)DB : (blockIdx.x == (cut >> 8) ? (cut & 0xffu) : 0u);
    uint32_t tot;
    const uint32_t ex = dvs_block_excl_scan((a != DVS_DENSIFY_PRUNE ? 1u : 0u) | (d_grows(a) ? 1u << 16 : 0u), tmp, &tot);
    const uint32_t rank = ex >> 16;                                  // growth candidates before i in this block
    if (d_grows(a) && rank >= quota) { a = DVS_DENSIFY_KEEP; action[i] = (uint8_t)a; }
    if (i < n) offsets[i] = block_offsets[blockIdx.x] + (ex & 0xffffu) + min(rank, quota);
}

// mode 0: parameters; mode 1: optimizer moments
__global__ void __launch_bounds__(DB)
k_densify_apply(int n, const uint8_t* __restrict__ action, const uint32_t* __restrict__ offsets, dvs_densify_params p, int mode,
                const float* __restrict__ s_pos, const float* __restrict__ s_sh0, const float* __restrict__ s_shn,
                const float* __restrict__ s_op, const float* __restrict__ s_sc, const float* __restrict__ s_rot,
                float* __restrict__ d_pos, float* __restrict__ d_sh0, float* __restrict__ d_shn, float* __restrict__ d_op,
                float* __restrict__ d_sc, float* __restrict__ d_rot, int new_n) {
    const int i = blockIdx.x * DB + threadIdx.x;
    if (i >= n) return;
    const int a = action[i];
    if (a == DVS_DENSIFY_PRUNE) return;
    const uint32_t o0 = offsets[i];
    const int copies = a == DVS_DENSIFY_KEEP ? 1 : 2;
    float pos[3], sc[3], q[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) { pos[k] = s_pos[3 * (int64_t)i + k]; sc[k] = s_sc[3 * (int64_t)i + k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = s_rot[4 * (int64_t)i + k];
    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (mode == 0 && a == DVS_DENSIFY_SPLIT) {
        const float qn = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        const float iq = qn > 0.f ? 1.0f / qn : 0.f;
        dvs_quat_to_rot(q[0] * iq, q[1] * iq, q[2] * iq, q[3] * iq, R);
    }
    for (int c = 0; c < copies; ++c) {
        const int j = (int)o0 + c;
        if (j >= new_n) break;
        const bool fresh = mode == 1 && !(a == DVS_DENSIFY_KEEP || (a == DVS_DENSIFY_CLONE && c == 0));   // moments of new splats = 0
        float np[3] = {pos[0], pos[1], pos[2]}, ns[3] = {sc[0], sc[1], sc[2]};
        if (mode == 0 && a == DVS_DENSIFY_SPLIT) {
            // sample from the splat's own Gaussian: pos + R diag(s) z, z ~ N(0, I); children shrink by 1.6
            float z[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) z[k] = d_normal(p.seed, (uint32_t)i, (uint32_t)(c * 3 + k)) * __expf(sc[k]);
#pragma unroll
            for (int r = 0; r < 3; ++r) np[r] = pos[r] + R[r * 3] * z[0] + R[r * 3 + 1] * z[1] + R[r * 3 + 2] * z[2];
#pragma unroll
            for (int k = 0; k < 3; ++k) ns[k] = sc[k] - 0.47000363f;     // log(1.6)
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            d_pos[3 * (int64_t)j + k] = fresh ? 0.f : np[k];
            d_sc[3 * (int64_t)j + k] = fresh ? 0.f : ns[k];
            d_sh0[3 * (int64_t)j + k] = fresh ? 0.f : s_sh0[3 * (int64_t)i + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) d_rot[4 * (int64_t)j + k] = fresh ? 0.f : q[k];
        float op = s_op[i];
        if (mode == 0 && p.revised_opacity && a != DVS_DENSIFY_KEEP) {        // o' = 1 - sqrt(1 - o) for both results
            const float o = 1.0f / (1.0f + __expf(-op));
            const float no = fminf(fmaxf(1.0f - sqrtf(1.0f - o), 1e-6f), 1.0f - 1e-6f);
            op = __logf(no / (1.0f - no));
        }
        d_op[j] = fresh ? 0.f : op;
        for (int e = 0; e < 45; ++e) d_shn[dvs_shn_index(p.shn_layout, j, e)] = fresh ? 0.f : s_shn[dvs_shn_index(p.shn_layout, i, e)];
    }
}

__global__ void __launch_bounds__(DB)
k_reset_opacity(int n, float* __restrict__ opacity, float logit_max, float* __restrict__ m, float* __restrict__ v) {
    const int i = blockIdx.x * DB + threadIdx.x;
    if (i >= n) return;
    opacity[i] = fminf(opacity[i], logit_max);
    if (m) m[i] = 0.f;
    if (v) v[i] = 0.f;
}

// ---- importance-scored pruning: exact selection of the splats a prune keeps (dvs_importance_plan) -------------------------------------
// The pruned splats are the p = n - min(keep, n) smallest in the total order (score, then larger index first). A most-significant-
// digit-first radix select over the 64-bit score finds the p-th smallest score S: eight rounds of (256-bin histogram of the next byte
// over the splats that match the bytes chosen so far | one workgroup picks the byte in which the rank falls). Every splat below S
// goes, every one above stays, and of the E splats equal to S the first E - r in index order stay (r = p - #{score < S}): the mark
// pass resolves that with one scan of the equal flags. No host round trip: rank, prefix and cut live in the scratch.
struct ImpState {
    unsigned long long prefix;     // the bytes of S chosen so far (the others zero); after the last round: S
    unsigned long long rank;       // 1-based rank of the p-th smallest among the splats that match the prefix; after the last round: r
    unsigned long long cut;        // splats equal to S that stay (E - r); n when nothing is pruned
};
#define IMP_HIST_WORDS (8 * 256)
// the scratch's three parts; a const scratch gives const parts (k_importance_mark only reads)
__device__ __forceinline__ const ImpState* imp_state(const void* scratch) { return (const ImpState*)scratch; }
__device__ __forceinline__ const uint32_t* imp_hist(const void* scratch) { return (const uint32_t*)((const char*)scratch + 32); }
__device__ __forceinline__ const uint32_t* imp_blocks(const void* scratch) { return imp_hist(scratch) + IMP_HIST_WORDS; }
__device__ __forceinline__ ImpState* imp_state(void* scratch) { return const_cast<ImpState*>(imp_state((const void*)scratch)); }
__device__ __forceinline__ uint32_t* imp_hist(void* scratch) { return const_cast<uint32_t*>(imp_hist((const void*)scratch)); }
__device__ __forceinline__ uint32_t* imp_blocks(void* scratch) { return const_cast<uint32_t*>(imp_blocks((const void*)scratch)); }

__global__ void __launch_bounds__(DB) k_importance_init(void* scratch, unsigned long long n, unsigned long long prune) {
    uint32_t* h = imp_hist(scratch);
    for (int k = threadIdx.x; k < IMP_HIST_WORDS; k += DB) h[k] = 0u;
    if (threadIdx.x == 0) { ImpState* s = imp_state(scratch); s->prefix = 0ull; s->rank = prune; s->cut = n; }
}
// round `round` (0 = the most significant byte): counts byte (score >> shift) & 255 of the splats whose higher bytes equal the prefix's
__global__ void __launch_bounds__(DB)
k_importance_hist(int n, const unsigned long long* __restrict__ score, void* scratch, int round) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 56 - 8 * round;
    const unsigned long long prefix = imp_state(scratch)->prefix;
    for (int64_t i = (int64_t)blockIdx.x * DB + threadIdx.x; i < n; i += (int64_t)gridDim.x * DB) {
        const unsigned long long k = score[i];
        if (round == 0 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&h[(uint32_t)(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t c = h[threadIdx.x];
    if (c) atomicAdd(&imp_hist(scratch)[round * 256 + threadIdx.x], c);
}
// one workgroup, thread = byte value: the byte g with #{byte < g} < rank <= #{byte <= g}
__global__ void __launch_bounds__(DB) k_importance_pick(void* scratch, int round) {
    __shared__ uint32_t tmp[DB / 64];
    ImpState* s = imp_state(scratch);
    const unsigned long long rank = s->rank;
    const uint32_t c = imp_hist(scratch)[round * 256 + threadIdx.x];
    uint32_t tot;
    const uint32_t below = dvs_block_excl_scan(c, tmp, &tot);               // (its barriers order the read of rank before the write below)
    if ((unsigned long long)below < rank && rank <= (unsigned long long)below + c) {             // exactly one thread: 1 <= rank <= tot
        s->prefix |= (unsigned long long)threadIdx.x << (56 - 8 * round);
        s->rank = rank - below;
        if (round == 7) s->cut = (unsigned long long)c - (rank - below);
    }
}
// per block: (splats below S) | (splats equal to S) << 16, both <= DB
__global__ void __launch_bounds__(DB)
k_importance_blocksum(int n, const unsigned long long* __restrict__ score, void* scratch) {
    __shared__ uint32_t tmp[DB / 64];
    const int i = blockIdx.x * DB + threadIdx.x;
    const unsigned long long S = imp_state(scratch)->prefix;
    const unsigned long long k = i < n ? score[i] : ~0ull;
    uint32_t tot;
    (void)dvs_block_excl_scan((i < n && k < S ? 1u : 0u) | (i < n && k == S ? 1u << 16 : 0u), tmp, &tot);
    if (threadIdx.x == 0) imp_blocks(scratch)[2 * blockIdx.x] = tot;
}
// single workgroup over the nb packed block sums, DB blocks per chunk with a running carry: per block the splats kept before it
// (its first index - those below S before it - those equal to S before it beyond the first `cut`) and the equal ones before it
__global__ void __launch_bounds__(DB) k_importance_scan_blocks(void* scratch, uint32_t nb, unsigned long long new_n, uint64_t* __restrict__ new_count) {
    __shared__ uint32_t tmp[DB / 64];
    uint32_t* blocks = imp_blocks(scratch);
    const unsigned long long cut = imp_state(scratch)->cut;
    unsigned long long cl = 0, ce = 0;
    for (uint32_t base = 0; base < nb; base += DB) {
        const uint32_t idx = base + threadIdx.x;
        const uint32_t v = idx < nb ? blocks[2 * idx] : 0u;
        uint32_t tl, te;
        const unsigned long long el = cl + dvs_block_excl_scan(v & 0xffffu, tmp, &tl);
        const unsigned long long ee = ce + dvs_block_excl_scan(v >> 16, tmp, &te);
        if (idx < nb) {
            blocks[2 * idx] = (uint32_t)((unsigned long long)idx * DB - el - (ee > cut ? ee - cut : 0ull));
            blocks[2 * idx + 1] = (uint32_t)ee;
        }
        cl += tl; ce += te;
    }
    if (threadIdx.x == 0) *new_count = new_n;
}
__global__ void __launch_bounds__(DB)
k_importance_mark(int n, const unsigned long long* __restrict__ score, const void* scratch, uint8_t* __restrict__ action,
                  uint32_t* __restrict__ offsets) {
    __shared__ uint32_t tmp[DB / 64];
    const int i = blockIdx.x * DB + threadIdx.x;
    const unsigned long long S = imp_state(scratch)->prefix, cut = imp_state(scratch)->cut;
    const uint32_t* blocks = imp_blocks(scratch);
    const unsigned long long k = i < n ? score[i] : 0ull;
    const bool equal = i < n && k == S;
    uint32_t tot;
    const uint32_t eq_before = blocks[2 * blockIdx.x + 1] + dvs_block_excl_scan(equal ? 1u : 0u, tmp, &tot);
    const bool kept = i < n && (k > S || (equal && (unsigned long long)eq_before < cut));
    const uint32_t ex = dvs_block_excl_scan(kept ? 1u : 0u, tmp, &tot);
    if (i < n) {
        action[i] = (uint8_t)(kept ? DVS_DENSIFY_KEEP : DVS_DENSIFY_PRUNE);
        offsets[i] = blocks[2 * blockIdx.x] + ex;
    }
}

extern "C" {
int dvs_densify_accumulate(void* stream, int n, const int32_t* radii, const float* absgrad2d, int width, int height, float* grad_accum,
                           float* denom, int32_t* max_radii) {
    if (n < 0 || (n > 0 && (!radii || !absgrad2d || !grad_accum || !denom || !max_radii))) return DVS_ERR_INVALID;
    if (n == 0) return DVS_OK;
    hipLaunchKernelGGL(k_densify_accumulate, dim3((n + DB - 1) / DB), dim3(DB), 0, (hipStream_t)stream, n, radii, (const float2*)absgrad2d,
                       0.5f * (float)width, 0.5f * (float)height, grad_accum, denom, max_radii);
    return dvs_launch_status();
}
int dvs_densify_accumulate_rows(void* stream, int n, int n_views, const int32_t* radii, const float* rows, int width, int height,
                                float* grad_accum, float* denom, int32_t* max_radii) {
    if (n < 0 || n_views < 1 || (n > 0 && (!radii || !rows || !grad_accum || !denom || !max_radii))) return DVS_ERR_INVALID;
    if (n == 0) return DVS_OK;
    hipLaunchKernelGGL(k_densify_accumulate_rows, dim3((n + DB - 1) / DB), dim3(DB), 0, (hipStream_t)stream, n, n_views, radii, rows,
                       0.5f * (float)width, 0.5f * (float)height, grad_accum, denom, max_radii);
    return dvs_launch_status();
}
int dvs_any_view_radius(void* stream, int n, int n_views, const int32_t* radii, int32_t* out) {
    if (n < 0 || n_views < 1 || (n > 0 && (!radii || !out))) return DVS_ERR_INVALID;
    if (n == 0) return DVS_OK;
    hipLaunchKernelGGL(k_any_view_radius, dim3((n + DB - 1) / DB), dim3(DB), 0, (hipStream_t)stream, n, n_views, radii, out);
    return dvs_launch_status();
}
int dvs_densify_plan(void* stream, int n, const float* opacity, const float* scale, const float* grad_accum, const float* denom,
                     const int32_t* max_radii, const dvs_densify_params* prm, uint8_t* action, uint32_t* offsets, uint32_t* scratch,
                     uint64_t* new_count) {
    if (n < 0 || !prm || !new_count || (n > 0 && (!opacity || !scale || !grad_accum || !denom || !max_radii || !action || !offsets || !scratch)))
        return DVS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nb = (uint32_t)((n + DB - 1) / DB);
    if (nb) hipLaunchKernelGGL(k_densify_blocksum, dim3(nb), dim3(DB), 0, st, n, opacity, scale, grad_accum, denom, max_radii, *prm, action, scratch);
    hipLaunchKernelGGL(k_densify_scan_blocks, dim3(1), dim3(DB), 0, st, scratch, nb, prm->cap_max, new_count);
    if (nb) hipLaunchKernelGGL(k_densify_offsets, dim3(nb), dim3(DB), 0, st, n, action, scratch, offsets);
    return dvs_launch_status();
}
int dvs_densify_apply(void* stream, int n, const uint8_t* action, const uint32_t* offsets, const dvs_densify_params* prm, int mode,
                      const float* const src[6], float* const dst[6], int new_n) {
    if (n < 0 || !prm || (n > 0 && (!action || !offsets || !src || !dst))) return DVS_ERR_INVALID;
    if (n == 0) return DVS_OK;
    hipLaunchKernelGGL(k_densify_apply, dim3((n + DB - 1) / DB), dim3(DB), 0, (hipStream_t)stream, n, action, offsets, *prm, mode, src[0], src[1],
                       src[2], src[3], src[4], src[5], dst[0], dst[1], dst[2], dst[3], dst[4], dst[5], new_n);
    return dvs_launch_status();
}
size_t dvs_importance_scratch_bytes(int n) {
    if (n <= 0) return 0;
    const size_t nb = ((size_t)n + DB - 1) / DB;
    return dvs_align256(32 + (IMP_HIST_WORDS + 2 * nb) * sizeof(uint32_t));
}
int dvs_importance_plan(void* stream, int n, const uint64_t* score, uint32_t keep, uint8_t* action, uint32_t* offsets, void* scratch,
                        uint64_t* new_count) {
    if (n <= 0 || keep == 0 || !score || !action || !offsets || !scratch || !new_count || ((uintptr_t)score & 7u) || ((uintptr_t)scratch & 15u) ||
        ((uintptr_t)new_count & 7u))
        return DVS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nb = (uint32_t)((n + DB - 1) / DB);
    const uint64_t kept = keep < (uint32_t)n ? keep : (uint32_t)n, prune = (uint64_t)n - kept;
    const unsigned long long* sc = (const unsigned long long*)score;
    hipLaunchKernelGGL(k_importance_init, dim3(1), dim3(DB), 0, st, scratch, (unsigned long long)n, (unsigned long long)prune);
    if (prune > 0)                                                        // (nothing pruned: S = 0 and cut = n keep every splat)
        for (int round = 0; round < 8; ++round) {
            hipLaunchKernelGGL(k_importance_hist, dim3(nb < 1024u ? nb : 1024u), dim3(DB), 0, st, n, sc, scratch, round);
            hipLaunchKernelGGL(k_importance_pick, dim3(1), dim3(DB), 0, st, scratch, round);
        }
    hipLaunchKernelGGL(k_importance_blocksum, dim3(nb), dim3(DB), 0, st, n, sc, scratch);
    hipLaunchKernelGGL(k_importance_scan_blocks, dim3(1), dim3(DB), 0, st, scratch, nb, (unsigned long long)kept, new_count);
    hipLaunchKernelGGL(k_importance_mark, dim3(nb), dim3(DB), 0, st, n, sc, (const void*)scratch, action, offsets);
    return dvs_launch_status();
}
int dvs_reset_opacity(void* stream, int n, float* opacity, float max_opacity, float* adam_m, float* adam_v) {
    if (n < 0 || (n > 0 && !opacity) || !(max_opacity > 0.f && max_opacity < 1.f)) return DVS_ERR_INVALID;
    if (n == 0) return DVS_OK;
    hipLaunchKernelGGL(k_reset_opacity, dim3((n + DB - 1) / DB), dim3(DB), 0, (hipStream_t)stream, n, opacity,
                       logf(max_opacity / (1.f - max_opacity)), adam_m, adam_v);
    return dvs_launch_status();
}
}
