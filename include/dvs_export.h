/*
 * dvs_export.h — C-ABI of the model export packers: the trained splats, as train_step() holds them on the device, packed into the
 * compact formats of DIVSHOT's viewer whose definition is open code (external/tinygsplat, external/spz):
 *   .compressed.ply  chunks of 256 splats, 48 B of bounds per chunk + 16 B per splat   tiny_gsplat.cpp:293-396 (save), :766-815 (load),
 *                    tiny_gsplat.hpp:342-534 (packUnorm, pack8888, packColor, SplatChunk::pack / unpack)
 *   .splat           one 32-byte record per splat                                       tiny_gsplat.cpp:243-291
 *   .spz             version 3: six byte sections, 20 + 3 dim B per splat, gzipped      spz/src/load-spz.cc (packGaussians,
 *                    by the host writer; the one compact format with the SH bands above 0       unpackGaussians), tiny_gsplat.cpp:1232-1272
 *   .reduced.ply     quantised: four per-degree vertex blocks of codebook ids + twenty           tiny_gsplat.cpp:398-630 (save), :817-992 (load);
 *                    256-entry k-means codebooks, 17..68 B per splat (last section below)        the producing side is defined in this header
 * Only the packed payload has to cross to the host (16.2 B / 32 B / 65 B per splat instead of the 236 B of the full PLY). The first two
 * never read the SH bands above 0 (neither format has them), so the layout of shN does not matter to them; .spz reads either layout.
 *
 * Conventions of dvs_train.h: `stream` is a hipStream_t, every array is a DEVICE pointer on a 16-byte boundary, the calls are
 * asynchronous and return a DVS_* status (dvs_raster.h). The parameter arrays are the raw pre-activation fp32 arrays of dvs_splats:
 * pos [n][3], sh0 [n][3], opacity [n] (logit), scale [n][3] (log), rot [n][4] (not normalised). No atomics anywhere: two calls on the
 * same inputs return identical bytes. All arithmetic below is fp32 without contraction unless it says otherwise.
 */
#ifndef DVS_EXPORT_H
#define DVS_EXPORT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of scratch dvs_pack_compressed needs for n splats (0 for n <= 0): the partial bounds, the sort's segment descriptor, histogram
 * table and digit totals, and the two (key, index) array pairs of the sort. No initialisation needed. */
size_t dvs_pack_scratch_bytes(int n);

/* The chunked, quantised PLY payload.
 *   order   the splats in Morton order: 30-bit keys, 10 bits per axis, q_a = (uint32)(rel_a * 1023.0f) with
 *           rel_a = ext_a < 1e-5f ? 0 : (p_a - min_a) / ext_a over the model's bounding box; bit i of q_x / q_y / q_z is key bit
 *           3i / 3i + 1 / 3i + 2; equal keys stay in index order (stable LSD radix sort, four passes). order[j] = model index of output
 *           vertex j. `order` may be NULL.
 *   chunks  [ceil(n / 256)][12] = {pmin xyz, pmax xyz, smin xyz, smax xyz}: bounds of pos and of the raw (log) scale over the chunk's
 *           own members, chunk c = output vertices [256 c, min(n, 256 c + 256)).
 *   verts   [n][4] in the order of the file's vertex properties:
 *             [0] packed_position  pack111011(norm(p_x), norm(p_y), norm(p_z))       11 / 10 / 11 bits at shifts 21 / 11 / 0
 *             [1] packed_rotation  largest << 30 | the other three components, 10 bits each, in index order:
 *                                  q = rot / sqrt(((r0^2 + r1^2) + r2^2) + r3^2) (a squared norm of 0 or not finite: q = (1, 0, 0, 0)),
 *                                  largest = first index of the greatest |q_i|, all four negated if q_largest < 0,
 *                                  each other one as packUnorm(q_i * 0.70710678f + 0.5f, 10)
 *             [2] packed_scale     pack111011 of the raw scale, normalised the same way
 *             [3] packed_color     pack8888(sh0_r C0 + 0.5f, sh0_g C0 + 0.5f, sh0_b C0 + 0.5f, sigmoid(opacity)), R in the top byte,
 *                                  C0 = 0.28209479177387814f
 *           norm(x) = (max - min < 0.00001f) ? 0 : (x - min) / (max - min);
 *           packUnorm(v, bits) = clamp(floor((double)(v * t) + 0.5), 0, t), t = 2^bits - 1.
 *   scratch dvs_pack_scratch_bytes(n) bytes.
 * DVS_ERR_INVALID for n <= 0, a NULL pointer other than `order`, a pointer off a 16-byte boundary. */
int dvs_pack_compressed(void* stream, int n, const float* pos, const float* sh0, const float* opacity, const float* scale,
                        const float* rot, void* scratch, float* chunks /*[ceil(n/256)][12]*/, uint32_t* verts /*[n][4]*/,
                        uint32_t* order /*nullable [n]: order[j] = model index of output vertex j*/);

/* The 32-byte .splat records, in the model's own order: bytes 0-11 pos as f32; 12-23 exp(scale) as f32; 24-26
 * (u8)clamp((0.5f + C0 sh0_c) * 255, 0, 255); 27 (u8)clamp(sigmoid(opacity) * 255, 0, 255); 28-31 (u8)clamp(q_i * 128 + 128, 0, 255)
 * over the normalised quaternion q of packed_rotation above. The conversions truncate (tiny_gsplat.cpp:268-277).
 * DVS_ERR_INVALID for n <= 0, a NULL pointer, a pointer off a 16-byte boundary. */
int dvs_pack_splat32(void* stream, int n, const float* pos, const float* sh0, const float* opacity, const float* scale,
                     const float* rot, uint8_t* out /*[n][32]*/);

/* ---- .spz, version 3 ----------------------------------------------------------------------------------------------------------------
 * The packed model is ONE device buffer holding the six sections in file order: positions (9 n bytes), alphas (n), colors (3 n),
 * scales (3 n), rotations (4 n), sh (3 dim n; dim = 0 / 3 / 8 / 15 coefficients per channel for degree 0 .. 3). Section k starts at
 * off[k], a multiple of 16, and has bytes[k] bytes; the bytes between a section's end and the next off[] are never written or read.
 * The file is the 16-byte header followed by the bytes[k] bytes of each section (gsply::write_spz). total = the buffer's size. */
typedef struct dvs_spz_layout { uint64_t off[6], bytes[6], total; } dvs_spz_layout;   /* positions, alphas, colors, scales, rotations, sh */
/* Host only. DVS_ERR_INVALID for n <= 0, a degree outside 0..3, out == NULL. */
int dvs_spz_layout_for(int n, int sh_degree, dvs_spz_layout* out);

/* packGaussians with PackOptions.from unspecified (every flip is 1), as save_spz_splats calls it. round() rounds halves away from zero;
 * u8(v) = (uint8)clamp(round(v), 0, 255).
 *   positions  per component f = round(p * 4096.0f) saturated to [-2^23, 2^23 - 1], three bytes, little-endian (12 fractional bits).
 *              [the reference keeps the low 24 bits of an out-of-range value; a p that is not finite is undefined there: 0 here]
 *   alphas     u8(sigmoid(opacity) * 255.0f), the library's deterministic exp.            [a NaN logit, undefined there: 0 here]
 *   colors     u8(sh0 * (0.15f * 255.0f) + (0.5f * 255.0f)), both constants fp32 products. [NaN, undefined there: 0 here]
 *   scales     u8((s + 10.0f) * 16.0f) of the raw log scale.                              [NaN, undefined there: 0 here]
 *   rotations  q = (x, y, z, w) of the repository's (w, x, y, z), divided by sqrt(((x^2 + y^2) + z^2) + w^2), correctly rounded sqrt
 *              and divisions [a squared norm of 0 or not finite, undefined there: q = (0, 0, 0, 1)]; largest = the first index of the
 *              strictly greatest |q_i|, negate = q_largest < 0; comp = largest, then for every other index ascending
 *              comp = comp << 10 | ((q_i < 0) ^ negate) << 9 | min(511, (uint32)(511.0f * (|q_i| / 0.70710678f) + 0.5f)); four bytes,
 *              little-endian.
 *   sh         splat-major, then coefficient-major, channel-minor: byte (i * dim + j) * 3 + c from shN element j * 3 + c of splat i
 *              (not the (p * 15 + j) + c of tiny_gsplat.cpp:1265-1267, an index slip). r = round(x * 128.0f) clamped to [-512, 512]
 *              [NaN, undefined there: 0], q = (int)r + 128, q = (q + b / 2) / b * b in C integer arithmetic with b = 8 for the first
 *              9 values of a splat and 16 for the rest, byte = clamp(q, 0, 255). Only the first 3 dim floats of a splat are read.
 *   shN        DVS_SHN_ROWS [n][45] or DVS_SHN_TILED (dvs_raster.h; whole 64-splat tiles must be allocated). NULL allowed at degree 0.
 * `out`: dvs_spz_layout_for(n, sh_degree).total bytes.
 * DVS_ERR_INVALID for n <= 0, a degree outside 0..3, an unknown layout, a NULL pointer (shN: only above degree 0), a pointer off a
 * 16-byte boundary; nothing is launched then. */
int dvs_pack_spz(void* stream, int n, int sh_degree, const float* pos, const float* sh0, const float* shN, int shn_layout,
                 const float* opacity, const float* scale, const float* rot, uint8_t* out);

/* unpackGaussians with UnpackOptions.to unspecified, from the same buffer:
 *   pos      (float)sign_extended_24 * (1.0f / 4096.0f)            scale    b / 16.0f - 10.0f
 *   opacity  log(a / (1.0f - a)), a = b / 255.0f: the bytes 0 and 255 give -inf and +inf as in the reference; the rasterizer's forward
 *            culls a splat whose alpha stays below 1 / 255 (-inf) and sigmoid(+inf) = 1 saturates at its 0.99 cap.
 *   sh0      ((b / 255.0f) - 0.5f) / 0.15f                          shN      (b - 128.0f) / 128.0f; the coefficients above the degree
 *            are 0, and in DVS_SHN_TILED so are the three pad floats and the lanes of the last tile past n (whole tiles are written).
 *   rot      unpackQuaternionSmallestThree: from the low bits up, index 3 down to 0 skipping `largest` = comp >> 30:
 *            q_i = (0.70710678f * (float)(bits & 511)) / 511.0f, negated if bit 9 is set; sum += q_i^2 in that order starting from 0;
 *            q_largest = sqrt(1.0f - sum); written as (w, x, y, z).
 * shN may be NULL at degree 0 (nothing is written for it). Same DVS_ERR_INVALID rules as dvs_pack_spz. */
int dvs_unpack_spz(void* stream, int n, int sh_degree, const uint8_t* packed, float* pos, float* sh0, float* shN, int shn_layout,
                   float* opacity, float* scale, float* rot);

/* ---- .reduced.ply, the quantised variant (tiny_gsplat.cpp save_reduced_ply / load_reduced_ply with quantised = true) -----------------
 * Four vertex blocks, one per SH degree 0..3, then a table of twenty 256-entry scalar codebooks. The reference defines the container
 * and its reader; it has no caller that chooses degrees or builds codebooks, so the producing side is defined HERE, bit for bit
 * (tests/reduced_ply_ref.py restates it in numpy).
 * Codebook columns, in the file's order: 0 f_dc, 1..15 f_rest_0..14, 16 opacity, 17 scale, 18 rot_re, 19 rot_im. */
#define DVS_REDUCED_BOOKS 20
#define DVS_REDUCED_ENTRIES 256
#define DVS_REDUCED_MAX_VALUES (1 << 25)      /* values of one codebook: 3 n <= 2^25 */

/* Bytes of scratch the three calls below that take `scratch` need for n splats (0 for n <= 0). No initialisation needed. */
size_t dvs_reduced_scratch_bytes(int n);

/* degree[i] = the smallest SH degree k <= D that loses at most t of colour from any of the C camera centres (the cullSH rule).
 * For camera c: v = pos_i - o_c, len = sqrt((v_x^2 + v_y^2) + v_z^2), d = v / len; a camera with len == 0 or not finite is skipped.
 * err_k(i) = max over cameras and the three channels of |sum over the coefficients l of the bands k < band <= D of Y_l(d) shN[i][l][ch]|,
 * Y_l the basis of the rasterizer's forward (dvs_device.h constants); err_D = 0. degree[i] = the smallest k with err_k(i) <= t; an
 * err_k that is not finite exceeds t. fp32 without contraction; per channel the band sums are taken coefficient by coefficient in
 * ascending order and the bands added from the highest down (the result is a tolerance-level quantity: only its order of magnitude
 * matters). Every given camera counts and no visibility test is made: a camera that never sees the splat can only RAISE its degree,
 * so the rule is conservative. One lane per splat, no atomics.
 *   cams   DEVICE [C][3] camera centres         degree  DEVICE [n] bytes
 * DVS_ERR_INVALID for n <= 0, D outside 0..3, C <= 0, t negative or NaN, an unknown layout, a NULL pointer (shN: only above D = 0), a
 * pointer off a 16-byte boundary; nothing is launched then. */
int dvs_sh_degree_select(void* stream, int n, int D, const float* pos, const float* shN, int shn_layout, const float* cams, int C, float t,
                         uint8_t* degree);

/* The twenty codebooks of a model whose per-splat degrees are degree[] (each 0..3; a larger byte counts as 3).
 * Value sets (the STORED parameters, not activated): f_dc the 3 n sh0 values; f_rest_j the 3 channels of coefficient j of every splat
 * whose degree stores coefficient j (j < (degree + 1)^2 - 1); opacity the n logits; scale the 3 n log scales; rot_re / rot_im the w /
 * the x, y, z of rot normalised as dvs_pack_compressed normalises it: divided by sqrt(((w^2 + x^2) + y^2) + z^2), squared norm 0 or not
 * finite: (1, 0, 0, 0). (dvs_pack_spz sums w^2 last; the two can differ in the last bit.) A value that is not finite is clustered as 0,
 * and -0 as +0.
 * Per codebook, with V the multiset of its m values — the result does not depend on the order of V:
 *   1. m = 0, or A = max |v| = 0: all 256 centres are 0 (0 iterations).
 *   2. e = the exponent with A < 2^e <= 2 A (frexp); k(v) = (int64)rint(ldexp((double)v, 36 - e)), ties to even.
 *   3. s[0..m) = V ascending; c_j = s[((2 j + 1) m) / 512] (integer division), j = 0..255.
 *   4. One iteration: b_j = ((double)c_j + (double)c_{j+1}) * 0.5, j = 0..254; the cluster of v is #{j : b_j < (double)v} (a value on a
 *      boundary goes below it); c_q = (float)ldexp((double)S_q / (double)N_q, e - 36) with S_q the exact int64 sum of k(v) over cluster q
 *      and N_q its size; an empty cluster keeps its centre.
 *   5. Iterate until an iteration would assign every value as the one before it did (that iteration is not run or counted), at most
 *      max_iters iterations. iters[b] = the iterations run.
 *   6. The id of a value (dvs_pack_reduced) = its cluster by rule 4 under the FINAL centres.
 * Implementation: one stable radix sort of the order-preserving keys per codebook, an inclusive int64 prefix sum of k over s[], then all
 * iterations in ONE launch of ONE 256-lane workgroup (lane j owns centre j: 255 binary searches into s[] and prefix differences per
 * iteration). No float atomics, no host round trip; two calls give identical bytes. The codebooks are processed one after another.
 *   centres DEVICE [20][256] floats (book-major)     iters DEVICE [20] int32     scratch dvs_reduced_scratch_bytes(n) bytes
 * DVS_ERR_INVALID for n <= 0, 3 n > DVS_REDUCED_MAX_VALUES, max_iters < 1, an unknown layout, a NULL pointer (shN included), a pointer
 * off a 16-byte boundary; nothing is launched then. */
int dvs_codebooks_build(void* stream, int n, const float* sh0, const float* shN, int shn_layout, const float* opacity, const float* scale,
                        const float* rot, const uint8_t* degree, int max_iters, void* scratch, float* centres, int32_t* iters);

/* counts[d] (DEVICE, 4 words) = the number of splats of degree d (a byte above 3 counts as 3): what dvs_reduced_layout_for needs. */
int dvs_reduced_degree_counts(void* stream, int n, const uint8_t* degree, void* scratch, uint32_t* counts);

/* The payload = the file's bytes after end_header: block d at off[d] holds count[d] records of stride[d] = xyz + 3 + 3 coeffs + 8 bytes
 * (xyz = 12, or 6 with half; coeffs = (d + 1)^2 - 1), blocks back to back; the codebook table at table_off = off[3] + count[3] *
 * stride[3] is [256][20] floats (row = entry); total = table_off + 20480. */
typedef struct dvs_reduced_layout { uint64_t count[4], off[4], stride[4], table_off, total; int32_t half, _pad; } dvs_reduced_layout;
/* Host only. DVS_ERR_INVALID for counts == NULL, out == NULL, a sum of counts that is 0 or above INT32_MAX, half outside 0..1. */
int dvs_reduced_layout_for(const uint32_t counts[4], int half, dvs_reduced_layout* out);

/* The payload of L into `out` (L->total bytes). The record of a degree-d splat: xyz as 3 floats, or (L->half) as 3 halves — round to
 * nearest even, |x| >= 65520 (infinities included) saturates to +-65504, NaN -> 0; the 3 f_dc ids; the 3 coeffs f_rest ids, coefficient-
 * major and channel-minor; then opacity id, 3 scale ids, rot_re id, 3 rot_im ids. Ids by rule 6 above (binary search over the 255
 * boundaries of each codebook, held in LDS). Within a block the splats keep the model's order (a stable 4-way partition). L->count must
 * be the counts of degree[]: a record that would fall outside its block is not written. A workgroup stages its 256 splats' four runs
 * in LDS and stores them as 16-byte words wherever a run covers one.
 * DVS_ERR_INVALID for n <= 0 or n != the sum of L->count, an unknown layout, a NULL pointer (shN included), a pointer off a 16-byte
 * boundary; nothing is launched then. */
int dvs_pack_reduced(void* stream, int n, const float* pos, const float* sh0, const float* shN, int shn_layout, const float* opacity,
                     const float* scale, const float* rot, const uint8_t* degree, const float* centres /*[20][256]*/, void* scratch,
                     const dvs_reduced_layout* L, uint8_t* out);

/* What load_reduced_ply reconstructs from that payload, into a parameter set: the splats in BLOCK order (all of degree 0, then 1, ...),
 * every value the centre its id names (rot = (rot_re centre, three rot_im centres)), the coefficients above a splat's degree 0, and in
 * DVS_SHN_TILED so are the three pad floats and the lanes of the last tile past n (whole tiles are written). degree (nullable) [n]
 * receives each output splat's degree. Same DVS_ERR_INVALID rules as dvs_pack_reduced. */
int dvs_unpack_reduced(void* stream, int n, const uint8_t* packed, const dvs_reduced_layout* L, float* pos, float* sh0, float* shN,
                       int shn_layout, float* opacity, float* scale, float* rot, uint8_t* degree);

/* ---- export in a chosen frame: a similarity transform of the model (csrc/transform.hip; tests/transform_ref.py restates it) ------------
 * p' = s R p + t, R row-major. A splat under it: the position moves, the log scale gains log s, the quaternion is composed with R's,
 * the 45 higher SH floats are rotated band by band; sh0 and opacity are invariant. Non-uniform scale and shear cannot be represented
 * by a splat and have no entry here. */
typedef struct dvs_similarity { float R[9]; float t[3]; float s; } dvs_similarity;

/* HOST helpers: pure functions, no device, no statics. Each returns DVS_ERR_INVALID (nothing is written) for a NULL pointer, a
 * non-finite input, s <= 0, or an R that is not a rotation: ||R R^T - I||_inf (the largest absolute row sum) > 1e-4 or det < 0.
 *   dvs_similarity_from_trs  R = Rz(euler[2]) Ry(euler[1]) Rx(euler[0]), radians: the convention of dvs_region_from_trs (dvs_region.h),
 *                            formed in fp64 through the same half-angle quaternion and rounded once.
 *   dvs_similarity_inverse   s' = 1 / s, R' = R^T, t' = -(R^T t) / s, in fp64, rounded once.
 *   dvs_sh_rotation          D = the three band matrices 3x3, 5x5, 7x7, row-major, one after the other (9 + 25 + 49 = 83 floats), of THIS
 *                            library's real SH basis (dvs_sh_basis of the rasterizer's forward, its signs included): for every unit d and
 *                            every band, sum_k (D c)_k Y_k(R d) = sum_k c_k Y_k(d). Solved in fp64 by projection over a fixed set of
 *                            directions and rounded once to fp32. */
int dvs_similarity_from_trs(const float t[3], const float euler_rad[3], float s, dvs_similarity* out);
int dvs_similarity_inverse(const dvs_similarity* in, dvs_similarity* out);
int dvs_sh_rotation(const float R[9], float D[83]);

/* The model under a similarity, ONE launch. Every result is defined operation by operation in fp32 without contraction:
 *   pos'    row k: (((R[3k] x + R[3k+1] y) + R[3k+2] z) * s) + t[k]
 *   scale'  scale + ls, ls = (float)log((double)s), taken once on the host
 *   rot'    a (x) q, the Hamilton product in the stored (w, x, y, z) order, a = the unit quaternion of R (formed on the host in fp64 by the
 *           largest-diagonal branch, sign w >= 0 where w is the pivot, rounded once), q the splat's own quaternion, NOT normalised:
 *             w' = ((aw qw - ax qx) - ay qy) - az qz        x' = ((aw qx + ax qw) + ay qz) - az qy
 *             y' = ((aw qy - ax qz) + ay qw) + az qx        z' = ((aw qz + ax qy) - ay qx) + az qw
 *   shN'    per band l = 1..sh_degree and colour channel c, coefficient j of the band (element (first_l + j) * 3 + c, first_l = 0, 3, 8):
 *           D_l[j][0] v_0 + D_l[j][1] v_1 + ... summed left to right over v_k = element (first_l + k) * 3 + c. Bands above sh_degree are
 *           copied. In DVS_SHN_TILED whole tiles are written: the three pad floats and the lanes past n are 0 (the rule of dvs_unpack_spz).
 * In place is allowed: any *_out may equal its input (a lane touches only its own splat); other overlaps are not. D as dvs_sh_rotation
 * returns it for sim->R (it is not checked against R). shN / shN_out may be NULL at degree 0 (shN is then not touched). One wavefront
 * per 64-splat tile; sim and D are wave-uniform kernel arguments.
 * DVS_ERR_INVALID for n <= 0, a degree outside 0..3, an unknown layout, a NULL pointer (shN, shN_out: only above degree 0), a pointer
 * off a 16-byte boundary, a sim the host helpers would refuse; nothing is launched then. */
int dvs_transform_splats(void* stream, int n, int sh_degree, const dvs_similarity* sim, const float D[83], const float* pos, const float* shN,
                         int shn_layout, const float* scale, const float* rot, float* pos_out, float* shN_out, float* scale_out, float* rot_out);

/* Mesh vertices under the same similarity: xyz by the position rule; normals (nullable, then normals_out is ignored) by R alone,
 * ((R[3k] x + R[3k+1] y) + R[3k+2] z), not renormalised. [n][3] fp32 arrays of natural alignment; in place is allowed.
 * DVS_ERR_INVALID for n <= 0, NULL sim / xyz / xyz_out, normals without normals_out, a sim the host helpers would refuse. */
int dvs_transform_points(void* stream, int n, const dvs_similarity* sim, const float* xyz, const float* normals, float* xyz_out, float* normals_out);

/* ---- level of detail: moment-matched merging of the splats of every cell of a lattice (csrc/lod.hip; tests/lod_ref.py restates it) -------
 * A model with fewer splats that still covers the whole scene. The lattice: cell (ix, iy, iz) of a centre p is, per axis,
 * q = (p_a - origin_a) / cell (one subtraction, one IEEE division), 0 when !(q >= 0) (negative, NaN), dims_a - 1 when q >= dims_a, else
 * (uint32)q — the rule of dvs_mesh_decimate; key = (iz dims_y + iy) dims_x + ix < 2^30.
 *   dropped   a splat whose centre, opacity, scale or rotation holds a non-finite value (counted in n_dropped)
 *   weight    w_i = alpha_i (sigma0 sigma1 sigma2)^(2/3), formed as sigmoid(opacity) * exp(((s0 + s1) + s2) * (2/3)): opacity times a mean
 *             cross-section
 *   cluster   the surviving splats of one cell, in ascending splat index; every sum below is the serial sum in that order, from 0
 *   one member      its six rows are copied bit for bit (every SH band, whatever sh_degree)
 *   more members    W = sum w_i; !(W > 0): the cluster is dropped, its members counted in n_dropped. Else, in two passes,
 *             mu     = (sum w_i p_i) / W
 *             Sigma' = (sum w_i (Sigma_i + (p_i - mu)(p_i - mu)^T)) / W, Sigma_i = R_i diag(sigma_i^2) R_i^T of the unit quaternion
 *                      (dvs_unit_quat) as the rasterizer forms it, six components; a term is w_i * (Sigma_i[ab] + d_a * d_b)
 *             sh0, and every shN element of the bands <= sh_degree: (sum w_i c_i) / W; the bands above sh_degree: 0
 *             Sigma' = V diag(lambda) V^T by cyclic Jacobi sweeps (0,1), (0,2), (1,2) in fp32, at most 12, ended early only when the three
 *                      off-diagonal elements are exactly 0; lambda_k floored at 1e-7 max(lambda); scale'_k = 0.5 log(lambda_k)
 *             rot'   = the unit quaternion (w, x, y, z), w >= 0, of V with its third column negated when det V < 0
 *             alpha' = min(0.99, W / (lambda0 lambda1 lambda2)^(1/3)): the merged splat keeps the cluster's total weight; stored as its logit
 *   output    the live clusters in ascending cell key; m of them. A DVS_SHN_TILED output has zero pads and zero lanes past m.
 * Two calls, as the mesh decimation: _count sorts (ballot ranking), finds the clusters and returns counts = {m, n_dropped} (it
 * synchronises the stream); the caller allocates m rows (whole 64-splat tiles of shN for DVS_SHN_TILED); _write fills them from the same
 * scratch and inputs. exp and log are the device library's (a few ulp from libm's); nothing else is approximated. The only atomics are
 * integer additions to a counter: two runs return identical bytes. */
typedef struct dvs_lod_lattice { float origin[3]; float cell; int32_t dims[3]; } dvs_lod_lattice;

/* HOST: the lattice over a box bounds = {min xyz, max xyz} with `resolution` cells along its longest side: cell = (float)(longest * (1 +
 * 1e-5) / resolution) (the margin keeps the largest coordinate's quotient below `resolution`: it lands inside the last cell), origin =
 * the box's minimum, dims_a = ceil(side_a / cell), at least 1. DVS_ERR_INVALID (nothing is written) for a NULL pointer, a resolution
 * outside 4..1024, a non-finite bound, max < min on an axis, or a box without extent. */
int dvs_lod_lattice_for(const float bounds[6], int resolution, dvs_lod_lattice* out);

/* Bytes of scratch for n splats (256-byte aligned parts, no initialisation): the sort's workspace and arrays, the cluster tables, the
 * weights and the 48-byte records of dvs_lod_merge_write. */
size_t dvs_lod_scratch_bytes(int n);

/* counts = {m, n_dropped}. n = 0 gives {0, 0} and launches nothing. DVS_ERR_INVALID for n < 0, a NULL or misaligned pointer (16 bytes;
 * scratch: 256), a cell that is not a finite number > 0, a dims entry outside 1..1024, a non-finite origin. */
int dvs_lod_merge_count(void* stream, int n, const float* pos, const float* opacity, const float* scale, const float* rot,
                        const dvs_lod_lattice* lattice, void* scratch, uint32_t counts[2]);

/* The m merged splats, after dvs_lod_merge_count on the same n, inputs and scratch. The outputs must not overlap the inputs. n = 0
 * launches nothing. DVS_ERR_INVALID for a degree outside 0..3, an unknown layout, a NULL or misaligned pointer. */
int dvs_lod_merge_write(void* stream, int n, int sh_degree, const float* pos, const float* sh0, const float* shN, const float* opacity,
                        const float* scale, const float* rot, int shn_layout_in, const void* scratch, float* pos_out, float* sh0_out,
                        float* shN_out, float* opacity_out, float* scale_out, float* rot_out, int shn_layout_out);

#ifdef __cplusplus
}
#endif
#endif
