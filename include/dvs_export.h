/*
 * dvs_export.h — C-ABI of the model export packers: the trained splats, as train_step() holds them on the device, packed into the
 * compact formats of DIVSHOT's viewer whose definition is open code (external/tinygsplat, external/spz):
 *   .compressed.ply  chunks of 256 splats, 48 B of bounds per chunk + 16 B per splat   tiny_gsplat.cpp:293-396 (save), :766-815 (load),
 *                    tiny_gsplat.hpp:342-534 (packUnorm, pack8888, packColor, SplatChunk::pack / unpack)
 *   .splat           one 32-byte record per splat                                       tiny_gsplat.cpp:243-291
 *   .spz             version 3: six byte sections, 20 + 3 dim B per splat, gzipped      spz/src/load-spz.cc (packGaussians,
 *                    by the host writer; the one compact format with the SH bands above 0       unpackGaussians), tiny_gsplat.cpp:1232-1272
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

#ifdef __cplusplus
}
#endif
#endif
