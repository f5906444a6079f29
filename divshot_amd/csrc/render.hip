// render.hip — A7 alpha-composite forward for gfx950 (the composite backwards live in render_tr.hip and render_blocks.hip).
//
// One 16x16 tile per 256-thread workgroup = 4 wave64; each wave owns an 8x8 pixel quadrant so a
// splat's footprint can be rejected per wave. The tile's depth-ordered splat list is streamed
// through LDS in batches of 256 (one gathered splat per lane, then broadcast reads). k_render_fwd keeps the pixel predicates
// in scalar wave masks and runs the updates of a contributing pixel under EXEC = take (21 vector + 9 scalar instructions per visit), and
// writes per-tile live lists — the entries that reach the tile at all — for the default backward (render_tr.hip).
//
// Reference anchors (fenghuayumo/DIVSHOT): alpha rule and thresholds gsplat_ps.hlsl:60-65 (the viewer
// caps alpha at 0.999; the trainer constant fixed by this build is 0.99, SURVEY.md §8(a) A-notes),
// blend order renderer/gaussian.cpp:440, 16x16 groups gaussian_common.hlsl:162-163, abs-grad flag
// application/diverseshot-cli/source/main.cpp:44.
#include "dvs_device.h"
#include "dvs_kernels.h"
#include "render_common.h"

// ---- batch staging + per-quadrant culling masks -------------------------------------------------------
// Lane t of the workgroup gathers splat t of the batch into LDS and tests the ellipse on which the splat reaches
// alpha = 1/255 ( d^T Q d = 2 ln(255 o), Q = conic ) against the four 8x8 quadrants of the tile (exact
// ellipse-rectangle test). One ballot per quadrant turns the tests into 64-bit wave masks: the wave that
// owns quadrant q later walks only the set bits (s_ff1 / s_flbit, scalar unit) and never spends a vector
// instruction on a splat that cannot touch its pixels. The bound is inflated (1e-4 rel + 1e-3) and the rectangle minimum is
// computed from non-negative terms only (see stage_batch), so the exact per-pixel alpha test — unchanged — decides every
// contribution: results are identical to a full walk.
// A7's LDS layout: everything a visit reads sits at ONE address in three arrays — two ds_read_b128 and one ds_read_b32.
struct __attribute__((aligned(16))) FwdLds {
    float4 a[RB];       // mean x, mean y, cs.x, cs.y
    float4 b[RB];       // cs.z, opacity, colour r, colour g
    float4 c[RB];       // colour b in .x (16-B stride as the other two: one address register serves the three reads)
    uint64_t qmask[RB / 64][4];
    uint32_t wlive[RB / 64];    // entries of the batch that reach the tile at all, per wave (see the live lists in k_render_fwd)
};
// cs = (-0.5 log2e a, -log2e b, -0.5 log2e c): exp(power) = exp2(cs.x dx^2 + cs.y dx dy + cs.z dy^2)
__device__ __forceinline__ void lds_put(FwdLds& L, int t, float2 xy, float4 co, float3 col) {
    L.a[t] = make_float4(xy.x, xy.y, DVS_CS_SQ * co.x, DVS_CS_XY * co.y);
    L.b[t] = make_float4(DVS_CS_SQ * co.z, co.w, col.x, col.y);
    L.c[t].x = col.z;
}

// Returns the lane's entry: its splat id in `id_out` and whether it reaches any quadrant of the tile.
__device__ __forceinline__ bool stage_batch(FwdLds& L, const uint32_t* __restrict__ sorted_splat, uint32_t first, int cnt,
                                            const float4* __restrict__ splat2d, float tile_x0, float tile_y0, uint32_t& id_out) {
    const int t = threadIdx.x;
    uint32_t qm = 0;
    id_out = 0u;
    if (t < cnt) {
        const uint32_t id = sorted_splat[first + t];
        id_out = id;
        // the splat's 64-B record (dvs_fwd_state.splat2d): four 16-B loads from ONE cache line
        const float4 r0 = splat2d[4 * (size_t)id], r1 = splat2d[4 * (size_t)id + 1];
        const float4 r2 = splat2d[4 * (size_t)id + 2], r3 = splat2d[4 * (size_t)id + 3];     // colour b | .. | DVS_S2D_CULL constants
        const float bl = r2.x;
        const float2 xy = make_float2(r0.x, r0.y);
        const float4 co = make_float4(r0.z, r0.w, r1.x, r1.y);
        const float3 col = make_float3(r1.z, r1.w, bl);
        lds_put(L, t, xy, co, col);
        // The splat can reach alpha >= 1/255 only where q(d) = a dx^2 + 2 b dx dy + c dy^2 <= 2 ln(255 o), d = pixel - mean.
        // The minimum of the convex form over a quadrant's pixel rectangle is 0 if the mean lies inside, otherwise it lies on an edge
        // FACING the mean: the nearer vertical edge when the mean is left / right of the rectangle's columns, the nearer horizontal
        // edge when it is above / below. On the vertical line x:  q(x, y) = c (y - y*)^2 + x^2 det / c,  y* = -b x / c  (minimum at
        // y = clamp(y*, y0, y1)); every term is non-negative, so — unlike a x^2 + 2 b x y + c y^2 evaluated directly — nothing cancels
        // for thin, far-away splats, and det = a c - b^2 (which does cancel for them) is lowered by its own rounding bound: the
        // minimum is never over-estimated and the exact per-pixel test decides every contribution.
        // bound = 2 ln(255 o) inflated, det = a c - b^2 lowered by its rounding bound, det / c, det / a, -b / c, -b / a: per splat, from A2
        const float bound = r2.w;
        const float a = co.x, c = co.z;
        const float det_c = r3.x, det_a = r3.y, nb_c = r3.z, nb_a = r3.w;
        const float ox = tile_x0 - xy.x, oy = tile_y0 - xy.y;                 // tile origin relative to the mean
        float vy[2], vbase[2], hx[2], hbase[2];
        bool vin[2], hin[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float x0 = ox + 8.f * (float)i, x1 = x0 + 7.f, y0 = oy + 8.f * (float)i, y1 = y0 + 7.f;
            vin[i] = x0 <= 0.f && x1 >= 0.f; hin[i] = y0 <= 0.f && y1 >= 0.f;
            const float xe = x0 > 0.f ? x0 : x1, ye = y0 > 0.f ? y0 : y1;
            vy[i] = nb_c * xe; vbase[i] = vin[i] ? __builtin_inff() : xe * xe * det_c;
            hx[i] = nb_a * ye; hbase[i] = hin[i] ? __builtin_inff() : ye * ye * det_a;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = q & 1, row = q >> 1;
            const float x0 = ox + 8.f * (float)col, x1 = x0 + 7.f, y0 = oy + 8.f * (float)row, y1 = y0 + 7.f;
            const float ty_ = fminf(fmaxf(vy[col], y0), y1) - vy[col], tx_ = fminf(fmaxf(hx[row], x0), x1) - hx[row];
            const float ev = __builtin_fmaf(c * ty_, ty_, vbase[col]), eh = __builtin_fmaf(a * tx_, tx_, hbase[row]);
            const float qmn = (vin[col] && hin[row]) ? 0.f : fminf(ev, eh);
            qm |= !(qmn > bound) ? (1u << q) : 0u;                            // NaN-safe: a failed comparison keeps the splat
        }
    }
    const uint64_t m0 = __ballot(qm & 1u), m1 = __ballot(qm & 2u), m2 = __ballot(qm & 4u), m3 = __ballot(qm & 8u);
    if ((t & 63) == 0) {
        uint64_t* dst = L.qmask[t >> 6];
        dst[0] = m0; dst[1] = m1; dst[2] = m2; dst[3] = m3;
    }
    return qm != 0u;
}

__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// ---- A7 -------------------------------------------------------------------------------------------
// RECORD (dvs_debug_record_decisions, parity tests only): additionally stores, per (list position, 8x8 quadrant), the 64-bit mask of the
// pixels that TOOK the entry — the kernel's own threshold decisions — so that the fp64 oracle can be run on exactly these decisions
// (tests/test_gpu_parity.py: no "tainted" carve-out). Same arithmetic, same images.
template <bool RECORD>
__global__ void __launch_bounds__(RB)
k_render_fwd(ViewBg bg_arg /* MUST stay the first parameter: read through dvs_load_bg() */, int W, int H, int tiles_x, int tiles_per_view,
             int num_tiles /* = views * tiles_per_view */, const uint2* __restrict__ ranges, uint2* __restrict__ ranges_out /*null, or: `ranges` is the
             encoded form the tile sort's last pass leaves, and the (start, end) pairs go here*/,
             const uint32_t* __restrict__ sorted_splat, const float4* __restrict__ splat2d,
             float* __restrict__ out_color /*[views,3,H,W]*/, float* __restrict__ final_T /*[views,H,W]*/, uint32_t* __restrict__ n_contrib,
             uint32_t* __restrict__ live_splat /*[T] per tile, from ranges[tile].x: the entries that reach the tile, in list order*/,
             uint32_t* __restrict__ live_pos /*[T] per list position: how many entries before it (in its tile) reach the tile*/,
             uint64_t* __restrict__ take_masks /*RECORD: [capacity][4], zeroed by the caller*/, uint64_t take_cap) {
    __shared__ FwdLds L;
    (void)bg_arg;
    const int tile_g = tile_of_block(blockIdx.x, num_tiles);
    if (tile_g >= num_tiles) return;
    const int view = tile_g / tiles_per_view, tile = tile_g - view * tiles_per_view;
    const float3 bgv = dvs_load_bg(view);
    const float bg0 = bgv.x, bg1 = bgv.y, bg2 = bgv.z;
    out_color += (size_t)view * 3 * W * H; final_T += (size_t)view * W * H; n_contrib += (size_t)view * W * H;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int px = tx * DVS_TILE + (wave & 1) * 8 + (lane & 7);
    const int py = ty * DVS_TILE + (wave >> 1) * 8 + (lane >> 3);
    const bool inside = px < W && py < H;
    const float pxf = (float)px, pyf = (float)py;
    uint2 range = ranges[tile_g];
    if (ranges_out) {
        // A6 is fused into the tile sort's last pass (frontend.hip k_seg_scatter): the entry arrives as (~start, end), (0, 0) = no
        // instance. Decode it and leave the canonical pair — in its own array: no barrier between the waves' reads and this store — for
        // A8 and the exported state.
        range.x = range.y ? ~range.x : 0u;
        if (threadIdx.x == 0) ranges_out[tile_g] = range;
    }
    const int total = (int)(range.y - range.x);
    // Pixel state that decides control flow lives in wave masks (scalar registers): `notdone` = pixels still compositing. A visit forms
    // its predicates with three compares into masks, the scalar unit combines them, and the five updates of a contributing pixel
    // (three colour FMAs, T, last contributor) run under EXEC = `take` — no v_cndmask per visit, no branch either.
    uint64_t notdone = __builtin_amdgcn_ballot_w64(inside);
    float T = 1.0f, C0 = 0.f, C1 = 0.f, C2 = 0.f;
    uint32_t last = 0;
    // Live lists for the composite backward: 28 % of a C3 tile list are entries whose alpha >= 1/255 ellipse misses the tile (the 3-sigma
    // rectangle of A4 is wider). The staging test below already knows them; the entries that do reach the tile are written out compacted
    // (same order), with the map list position -> live position, so that A8 stages, tabulates and publishes 28 % fewer entries.
    uint32_t live_base = 0;

    for (int base = 0; base < total; base += RB) {
        if (__syncthreads_and(notdone == 0ull)) break;
        const int cnt = min(RB, total - base);
        uint32_t my_id;
        const bool live = stage_batch(L, sorted_splat, range.x + base, cnt, splat2d, (float)(tx * DVS_TILE), (float)(ty * DVS_TILE), my_id);
        const uint64_t lm = __ballot(live);
        const uint32_t lrank = __builtin_amdgcn_mbcnt_hi((uint32_t)(lm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)lm, 0u));
        if (lane == 0) L.wlive[wave] = (uint32_t)__popcll(lm);
        __syncthreads();
        if (live_pos) {
            uint32_t pre = 0, tot = 0;
#pragma unroll
            for (int w = 0; w < RB / 64; ++w) { const uint32_t c = L.wlive[w]; pre += w < wave ? c : 0u; tot += c; }
            const uint32_t lp = live_base + pre + lrank;
            if ((int)threadIdx.x < cnt) live_pos[range.x + base + threadIdx.x] = lp;
            if (live) live_splat[range.x + lp] = my_id;
            live_base += tot;
        }
        if (notdone == 0ull) continue;          // this wave's quadrant is finished
        // No per-lane branches (the scalar unit is shared by the CU's four SIMDs; a branchy body made this kernel scalar-bound); the
        // wave-uniform "everyone finished" exit is checked per 64-splat word.
#pragma unroll 1
        for (int lw = 0; lw < RB / 64; ++lw) {
            uint64_t m = uniform_u64(L.qmask[lw][wave]);
            if (m == 0) continue;
            if (notdone == 0ull) break;
            // LDS byte address of the word's first entry in a vector register (wave-uniform): a visit forms its address with ONE
            // v_lshl_add from the scalar bit index instead of s_or + s_lshl + v_mov
            typedef float fwd_v4f __attribute__((ext_vector_type(4)));
            typedef __attribute__((address_space(3))) const fwd_v4f lds_cv4f;
            uint32_t word_a = (uint32_t)(uintptr_t)&L.a[lw * 64];
            asm("" : "+v"(word_a));
            const int idx0 = base + lw * 64 + 1;
            // The visit below narrows EXEC and must leave it as it found it (not "-1" — a later per-lane branch around this
            // loop would otherwise get its dead lanes back): the entry mask is read once per word of the walk, not per visit.
            uint64_t exec_entry;
            asm volatile("s_mov_b64 %0, exec" : "=s"(exec_entry));
            while (m) {
                const int bit = __builtin_ctzll(m);
                asm("s_bitset0_b64 %0, %1" : "+s"(m) : "s"(bit));          // m &= m - 1 in one scalar instruction instead of three
                uint32_t ent_a;
                asm("v_lshl_add_u32 %0, %1, 4, %2" : "=v"(ent_a) : "s"(bit), "v"(word_a));
                const fwd_v4f A = *(lds_cv4f*)ent_a;
                const fwd_v4f B = *(lds_cv4f*)(ent_a + (uint32_t)sizeof(L.a));
                const float cb = *(const __attribute__((address_space(3))) float*)(ent_a + (uint32_t)(sizeof(L.a) + sizeof(L.b)));
                const float dx = A.x - pxf, dy = A.y - pyf;
                // log2 of the Gaussian falloff: p2 = log2e * power (sign unchanged), one v_exp_f32, no extra multiply
                const float p2 = __builtin_fmaf(B.x * dy, dy, __builtin_fmaf(A.w, dy, A.z * dx) * dx);
                const float alpha = fminf(DVS_ALPHA_MAX, B.y * __builtin_amdgcn_exp2f(p2));
                const float aT = alpha * T;
                const float test_T = T - aT;                       // = T (1 - alpha)
                const uint64_t nd_before = notdone;
                // The predicates as a v_cmpx chain: EXEC = notdone, narrowed by the two alpha-rule compares to the pixels the splat can
                // contribute to; the stop test runs under that mask (VCC = pixels that stop here, WITHOUT this splat), leaves `notdone`
                // and EXEC, and the five updates run on what is left. No mask ever travels through a scalar AND: 9 scalar instructions
                // per visit instead of 12 (the scalar unit is shared by the CU's four SIMDs).
                const uint32_t idx = (uint32_t)(idx0 + bit);
                asm volatile("s_mov_b64 exec, %[nd]\n\t"
                             "v_cmpx_nlt_f32_e32 vcc, 0, %[p2]\n\t"            // !(p2 > 0)
                             "v_cmpx_ngt_f32_e32 vcc, %[amin], %[al]\n\t"      // !(alpha < 1/255)
                             "v_cmp_gt_f32_e32 vcc, %[tstop], %[tt]\n\t"       // T (1 - alpha) < 1e-4: the pixel is done
                             "s_andn2_b64 %[nd], %[nd], vcc\n\t"
                             "s_andn2_b64 exec, exec, vcc\n\t"
                             "v_fmac_f32 %[c0], %[cr], %[at]\n\t"
                             "v_fmac_f32 %[c1], %[cg], %[at]\n\t"
                             "v_fmac_f32 %[c2], %[cbl], %[at]\n\t"
                             "v_sub_f32 %[T], %[T], %[at]\n\t"                 // (not a move of test_T: that one is a fused fma; same bits as the other A7 kernels)
                             "v_mov_b32 %[last], %[idx]\n\t"
                             "s_mov_b64 exec, %[ee]"
                             : [c0] "+v"(C0), [c1] "+v"(C1), [c2] "+v"(C2), [T] "+v"(T), [last] "+v"(last), [nd] "+s"(notdone)
                             : [p2] "v"(p2), [al] "v"(alpha), [tt] "v"(test_T), [cr] "v"(B.z), [cg] "v"(B.w), [cbl] "v"(cb), [at] "v"(aT), [idx] "s"(idx),
                               [amin] "s"(DVS_ALPHA_MIN), [tstop] "s"(DVS_T_STOP), [ee] "s"(exec_entry)
                             : "vcc", "scc");
                if (RECORD) {       // the same three comparisons on the same registers as the predicates above
                    const uint64_t took = nd_before & __builtin_amdgcn_ballot_w64(!(p2 > 0.f)) & __builtin_amdgcn_ballot_w64(!(alpha < DVS_ALPHA_MIN)) &
                                          ~__builtin_amdgcn_ballot_w64(test_T < DVS_T_STOP);
                    const uint64_t pos = (uint64_t)range.x + (uint64_t)(idx - 1u);
                    if (lane == 0 && pos < take_cap) take_masks[pos * 4 + wave] = took;
                }
            }
        }
    }
    if (inside) {
        const size_t P = (size_t)W * H, pix = (size_t)py * W + px;
        final_T[pix] = T;
        n_contrib[pix] = last;
        out_color[pix] = C0 + T * bg0;
        out_color[P + pix] = C1 + T * bg1;
        out_color[2 * P + pix] = C2 + T * bg2;
    }
}

// ---- launchers -----------------------------------------------------------------------------------------

hipError_t dvs_launch_render_fwd(hipStream_t st, int W, int H, int tiles_x, int tiles_y, int n_views, const uint32_t* ranges,
                                 const uint32_t* sorted_splat, const float* splat2d, const float* bgs, float* out_color, float* final_T,
                                 uint32_t* n_contrib, uint32_t* live_splat, uint32_t* live_pos, uint64_t* take_masks, uint64_t take_cap, uint32_t* ranges_out) {
    const int tiles_pv = tiles_x * tiles_y, num_tiles = tiles_pv * n_views;
    if (num_tiles <= 0) return hipSuccess;
    const int grid = replay_grid(num_tiles);
    if (take_masks)
        hipLaunchKernelGGL(k_render_fwd<true>, dim3(grid), dim3(RB), 0, st, make_view_bg(n_views, bgs), W, H, tiles_x, tiles_pv, num_tiles,
                           (const uint2*)ranges, (uint2*)ranges_out, sorted_splat, (const float4*)splat2d, out_color, final_T, n_contrib, live_splat, live_pos, take_masks, take_cap);
    else
        hipLaunchKernelGGL(k_render_fwd<false>, dim3(grid), dim3(RB), 0, st, make_view_bg(n_views, bgs), W, H, tiles_x, tiles_pv, num_tiles,
                           (const uint2*)ranges, (uint2*)ranges_out, sorted_splat, (const float4*)splat2d, out_color, final_T, n_contrib, live_splat, live_pos, (uint64_t*)nullptr, (uint64_t)0);
    return hipGetLastError();
}
