/*
 * dvs_export.h — C-ABI of the model export packers: the trained splats, as train_step() holds them on the device, packed into the two
 * compact formats of DIVSHOT's viewer whose definition is open code (external/tinygsplat):
 *   .compressed.ply  chunks of 256 splats, 48 B of bounds per chunk + 16 B per splat   tiny_gsplat.cpp:293-396 (save), :766-815 (load),
 *                    tiny_gsplat.hpp:342-534 (packUnorm, pack8888, packColor, SplatChunk::pack / unpack)
 *   .splat           one 32-byte record per splat                                       tiny_gsplat.cpp:243-291
 * Only the packed payload has to cross to the host (16.2 B / 32 B per splat instead of the 236 B of the full PLY). The SH bands above
 * 0 are never read (neither format has them), so the layout of shN does not matter.
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

#ifdef __cplusplus
}
#endif
#endif
