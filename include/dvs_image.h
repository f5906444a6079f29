/*
 * dvs_image.h — C-ABI of the image work on the device: the parallel half of baseline JPEG decoding (below), the parallel half of
 * baseline JPEG encoding (dvs_jpeg_encode_views, after it), the undistortion of a view taken through a distorted COLMAP camera
 * (dvs_undistort_view) and the parallel half of PNG decoding with the mask rule (dvs_png_reconstruct, dvs_mask_combine, at the end) and, right after that decoder, the parallel half of PNG encoding (dvs_png_encode_views).
 *
 * JPEG: quantised DCT coefficients (gstrain/jpeg_io.hpp decodes them on
 * the host) -> planar 8-bit RGB on the device, in one kernel: dequantisation, 8x8 inverse DCT, chroma upsampling, YCbCr -> RGB.
 *
 * Conventions of dvs_export.h: `stream` is a hipStream_t, the call is asynchronous and returns a DVS_* status (dvs_raster.h). No
 * scratch, no atomics: two calls on the same inputs return identical bytes. The result is defined bit for bit in integer arithmetic
 * (every intermediate fits int32 for every int16 coefficient and every quantiser up to 65535); tests/jpeg_ref.py restates it:
 *   dequantise   F = clamp(coef * q, -2048, 2047)        (an 8-bit image's DCT coefficients lie in [-1024, 1016] and a quantised one comes
 *                                                         back within q / 2 of its value: a real encoder's stream never clamps)
 *   inverse DCT  separable, direct matrix form, ONE table T[u][x] = round(2^13 * C(u) / 2 * cos((2x + 1) u pi / 16)), C(0) = 1 / sqrt(2),
 *                C(u > 0) = 1:   col[y][u] = (sum_v T[v][y] * F[v][u] + 2^8) >> 9      (columns first; 4 fractional bits are kept)
 *                                s[y][x]   = (sum_u col[y][u] * T[u][x] + 2^16) >> 17   (>> is the arithmetic shift)
 *                                sample    = clamp(s + 128, 0, 255)
 *   upsampling   the triangle filter common decoders apply by default, over the chroma plane cropped to cw = ceil(W / 2) columns (and, for
 *                2x2, ch = ceil(H / 2) rows); an index outside [0, cw - 1] or [0, ch - 1] is clamped into it (edge replication):
 *                2x1: out[2i] = (3 s[i] + s[i-1] + 1) >> 2,  out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2
 *                2x2: t[Y][i] = 3 s[Y>>1][i] + s[far][i],  far = (Y>>1) - 1 for even Y, (Y>>1) + 1 for odd Y;
 *                     out[Y][2i] = (3 t[Y][i] + t[Y][i-1] + 8) >> 4,  out[Y][2i+1] = (3 t[Y][i] + t[Y][i+1] + 7) >> 4
 *   colour       R = clamp(Y + ((91881 (Cr-128) + 32768) >> 16)),  B = clamp(Y + ((116130 (Cb-128) + 32768) >> 16)),
 *                G = clamp(Y + ((-22554 (Cb-128) - 46802 (Cr-128) + 32768) >> 16));  a grayscale image writes R = G = B = Y
 */
#ifndef DVS_IMAGE_H
#define DVS_IMAGE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct dvs_jpeg_desc {
    int32_t width, height;          /* 1 .. 65500 */
    int32_t components;             /* 1 (grayscale) or 3 (Y, Cb, Cr; the chroma components are sampled 1x1) */
    int32_t hs, vs;                 /* luma sampling: 1x1, 2x1 or 2x2 (1x1 when components = 1) */
    int32_t blocks_w[3], blocks_h[3];   /* per component: 8x8 blocks per row / per column, padded to whole MCUs:
                                           blocks_w = ceil(width / (8 hs)) * (hs for luma, 1 for chroma), blocks_h likewise */
    int32_t _pad;
    uint64_t offset[3];             /* per component: index of its first coefficient in `coef`, a multiple of 8 */
    uint16_t quant[3][64];          /* per component: the quantiser table in natural order (index 8 v + u) */
} dvs_jpeg_desc;

/* rgb = the image of `coef` (component-major, block-row-major, 64 natural-order coefficients per block, as gsjpeg::Frame holds them).
 * `desc` is a HOST pointer, read before the call returns; `coef` is a DEVICE pointer on a 16-byte boundary; `rgb` is a DEVICE pointer
 * to planar [3][height][width] bytes with no alignment requirement: rows leave as 16-byte stores when rgb is on a 16-byte boundary
 * and width is a multiple of 16, as single bytes otherwise, the same bytes either way.
 * DVS_ERR_INVALID for a NULL pointer, coef off a 16-byte boundary, or a desc that contradicts itself (sizes, sampling, block counts,
 * offsets that are no multiple of 8). */
int dvs_jpeg_reconstruct(void* stream, const dvs_jpeg_desc* desc, const int16_t* coef, uint8_t* rgb);

/* ---- encoding: planar fp32 RGB (what dvs_raster_forward_views writes) -> quantised DCT coefficients, the mirror image of the above;
 * gstrain/jpeg_write.hpp Huffman-codes them on the host. One launch takes up to DVS_JPEG_ENCODE_MAX_VIEWS views of one size. No
 * scratch, no atomics: two calls return identical bytes, and a view's output does not depend on the other views of the call. The
 * result is defined bit for bit; after the first step it is integer arithmetic in which every intermediate fits int32;
 * tests/jpeg_enc_ref.py restates it:
 *   float to byte  b = (int)min(255, max(0, rint(x * 255))): the fp32 product rounded to the nearest integer, ties to even; NaN -> 0.
 *                  This is the rule by which the trainer keeps 8-bit training views (GSPackLevel::PackF32ToU8), not the
 *                  truncation of x * 255 + 0.5: a render and its target are quantised alike. The two differ only on ties.
 *   padding        columns >= W and rows >= H up to the MCU grid repeat column W - 1 / row H - 1
 *   colour         Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *                  Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16
 *                  Cr = ( 32768 R - 27439 G -  5329 B + 8388608 + 32767) >> 16      (16-bit BT.601, the forward counterpart of the
 *                                                                                      decoder's constants; each lands in 0..255)
 *   subsampling    2x2: chroma sample (i, j) = (c[2j][2i] + c[2j][2i+1] + c[2j+1][2i] + c[2j+1][2i+1] + 2) >> 2 — inside the MCU
 *   forward DCT    s = sample - 128, the decoder's table T[u][x], rows first, SEVEN fractional bits kept between the passes and SIX
 *                  kept in F, which is the coefficient in 1/64 units (rounding F to an integer first and dividing by a small q
 *                  afterwards would round twice: at q = 2 every true |F| in [0.5, 1) would become 1):
 *                                row[y][u] = (sum_x T[u][x] * s[y][x] + 2^5) >> 6          (|row| <= 46336 < 2^17)
 *                                F[v][u]   = (sum_y T[v][y] * row[y][u] + 2^13) >> 14      (|sum| <= 23168 * 46336 < 2^31; |F| < 2^16 + 2^6)
 *   quantisation   c = sign(F) * (((|F| + 32 q) >> 6) / q)  (integer division; equal to (|F| + 64 q / 2) / (64 q): half away from zero
 *                  of the coefficient with its fraction), then clamp to [-1023, 1023], what a baseline Huffman stream can carry
 *                  (only a DC of -1024 at q = 1 ever meets the clamp) */
#define DVS_JPEG_ENCODE_MAX_VIEWS 16
#define DVS_JPEG_SAMPLING_420 0     /* hs = vs = 2 */
#define DVS_JPEG_SAMPLING_444 1     /* hs = vs = 1 */

/* host only: the descriptor of a width x height encode: three components, the sampling's block counts, the components one after the
 * other from offset 0, and the two Annex K quantiser tables (K.1 for Y, K.2 for Cb and Cr) scaled by the IJG quality rule
 * (scale = 5000 / quality below 50, 200 - 2 quality from 50 on; q = (base * scale + 50) / 100 clamped to 1..255).
 * DVS_ERR_INVALID for a NULL desc, a side outside 1..65500, another sampling, a quality outside 1..100. */
int dvs_jpeg_encode_desc(int width, int height, int sampling, int quality, dvs_jpeg_desc* desc);

/* host only: int16 values one view's coefficients take (the end of the last component); 0 for a desc dvs_jpeg_encode_views refuses */
size_t dvs_jpeg_encode_coef_count(const dvs_jpeg_desc* desc);

/* coef[v] = the coefficients of images[v], v < n_views, in the layout dvs_jpeg_reconstruct reads (padding blocks included). `desc`,
 * `images` and `coef` are HOST pointers, read before the call returns; images[v] is a DEVICE pointer to planar [3][height][width] fp32
 * with no alignment requirement beyond a float's: rows are read with 16-byte loads when every images[v] is on a 16-byte boundary and
 * width is a multiple of 4, element by element otherwise, the same bytes either way; coef[v] is a DEVICE pointer on a 16-byte
 * boundary to dvs_jpeg_encode_coef_count(desc) values; a block row of 8 coefficients leaves as one 16-byte store.
 * DVS_ERR_INVALID for a NULL pointer, n_views outside 1..16, a coef[v] off a 16-byte boundary, or a desc that contradicts itself
 * (sizes, components other than 3, a sampling other than 1x1 / 2x2, block counts, offsets that are no multiple of 8 or make two
 * components overlap, a quantiser outside 1..255). */
int dvs_jpeg_encode_views(void* stream, const dvs_jpeg_desc* desc, const float* const* images, int16_t* const* coef, int n_views);

/* ---- undistortion: a view of a SIMPLE_RADIAL, RADIAL or OPENCV camera -> the view of the pinhole camera that keeps its fx, fy, cx, cy
 * and its W x H. Coefficients a model lacks are 0; a pixel centre is at (x + 0.5, y + 0.5), COLMAP's convention. The ten floats of
 * the descriptor are each rounded ONCE from the doubles (the reciprocals ifx = 1 / fx, ify = 1 / fy are taken in double). Per target
 * pixel (x, y), in fp32, every `*` and `+` a separate round-to-nearest operation in the written order and bracketing (the file is
 * compiled without contraction), no division, no transcendental function; tests/undistort_ref.py restates it:
 *   u  = (((float)x + 0.5f) - cx) * ifx          v  = (((float)y + 0.5f) - cy) * ify
 *   u2 = u*u   v2 = v*v   uv = u*v   r2 = u2 + v2
 *   rad = (k1 + k2*r2) * r2
 *   du = (u*rad + (2.0f*p1)*uv) + p2*(r2 + 2.0f*u2)
 *   dv = (v*rad + (2.0f*p2)*uv) + p1*(r2 + 2.0f*v2)
 *   xs = (fx*(u + du) + cx) - 0.5f               ys = (fy*(v + dv) + cy) - 0.5f        (source index coordinates)
 *   in range  iff  xs > -1 && xs < W && ys > -1 && ys < H      (a NaN fails; only then is anything converted to int)
 *   qx = (int)floorf(xs*32.0f + 0.5f)            qy likewise                            (1/32-pixel fixed point)
 *   valid  iff  in range && 0 <= qx <= 32*(W-1) && 0 <= qy <= 32*(H-1)
 *   x0 = qx >> 5, ax = qx & 31, x1 = min(x0+1, W-1);   y0, ay, y1 likewise
 *   out = ((32-ax)*(32-ay)*s[y0][x0] + ax*(32-ay)*s[y0][x1] + (32-ax)*ay*s[y1][x0] + ax*ay*s[y1][x1] + 512) >> 10     per plane, integers
 * An invalid pixel writes 0 to every plane and 0 to the mask. A source mask (bytes in {0, 1}, the source image's geometry) goes through
 * the same integer formula as 255 m; the pixel is trainable iff the result is > 127. The output mask is 1.0f iff the pixel is valid and
 * trainable (without a source mask: iff valid), else 0.0f. Zero coefficients reproduce the source byte for byte with every pixel
 * valid: validity is decided on qx, not on xs. */
typedef struct dvs_undistort_desc { int32_t width, height; float fx, fy, cx, cy, ifx, ify, k1, k2, p1, p2; } dvs_undistort_desc;

/* host only: COLMAP model id 2 (SIMPLE_RADIAL: f cx cy k), 3 (RADIAL: f cx cy k1 k2) or 4 (OPENCV: fx fy cx cy k1 k2 p1 p2) and its
 * parameter doubles -> desc; DVS_ERR_INVALID for another model, a NULL pointer, a parameter that is not finite (as a double or once
 * rounded to fp32, the reciprocals included), f <= 0, a side outside 1..65536 */
int dvs_undistort_desc_from_colmap(int model, const double* params, int width, int height, dvs_undistort_desc* out);

/* src, dst: DEVICE planar [planes][H][W] bytes, planes 1..4, no alignment requirement, dst must not overlap src: the four bytes a lane
 * owns leave as one dword store when dst is on a 4-byte boundary and W is a multiple of 4, as single bytes otherwise, the same bytes
 * either way. mask_src: nullable DEVICE [H][W] bytes in {0,1}; mask_dst: nullable DEVICE [H][W] floats (16-byte stores when it is on a
 * 16-byte boundary and W is a multiple of 4); invalid_count: nullable DEVICE uint32, INCREMENTED by the number of invalid pixels (the
 * caller zeroes it; one atomic per wavefront that has any — an integer sum, so the count does not depend on their order).
 * `desc` is a HOST pointer, read before the call returns. No scratch; two calls on the same inputs return identical results.
 * DVS_ERR_INVALID for a NULL desc / src / dst, planes outside 1..4, a side outside 1..65536, dst overlapping src. */
int dvs_undistort_view(void* stream, const dvs_undistort_desc* desc, int planes, const uint8_t* src, const uint8_t* mask_src,
                       uint8_t* dst, float* mask_dst, uint32_t* invalid_count);

/* ---- PNG: filtered scanlines (gstrain/png_io.hpp inflates them on the host) -> planar 8-bit RGB and, when asked, alpha. Two launches:
 * the five filters undone in place, then sample expansion. No scratch, no atomics: two calls on the same inputs return identical bytes.
 * The result is defined bit for bit; tests/png_ref.py restates it:
 *   stream       per row one filter byte and rowbytes = ceil(W * channels * depth / 8) bytes; channels = 1 (types 0, 3), 2 (4), 3 (2), 4 (6)
 *   unfiltering  bpp = max(1, channels * depth / 8); x = the filtered byte, a = the byte bpp to the left, b = the byte above, c = the byte
 *                above a; bytes left of the row and the row above the first read as 0; every sum is taken modulo 256:
 *                0 None x | 1 Sub x + a | 2 Up x + b | 3 Average x + ((a + b) >> 1) (the 9-bit sum) |
 *                4 Paeth x + (p = a + b - c; pa = |p - a|, pb = |p - b|, pc = |p - c|; a if pa <= pb and pa <= pc, else b if pb <= pc, else c)
 *                a filter byte above 4 counts as None (the host half refuses such files)
 *   samples      depths 1, 2, 4: packed MSB first, each row padded to a byte, scaled by 255, 85, 17; depth 16: big-endian,
 *                byte = (v * 255 + 32895) >> 16; a palette index (type 3) goes through the 256-entry table
 *   colour       gray is written to all three planes; colour is stored as it is in the file, not premultiplied
 *   alpha        the alpha channel (types 4, 6), the palette table's alpha (type 3), or the colour key (types 0 and 2 with has_key):
 *                0 where every sample equals its key at the file's full depth (the key's bits above the depth are ignored), else 255;
 *                255 everywhere otherwise */
#define DVS_PNG_BAND 512               /* rows of one band of the unfiltering wavefront (the kernel's workgroup size) */
typedef struct dvs_png_desc {
    int32_t width, height;          /* 1 .. 65500 */
    int32_t bit_depth, color_type;  /* a legal PNG pair: type 0 at 1/2/4/8/16, 2 at 8/16, 3 at 1/2/4/8, 4 at 8/16, 6 at 8/16 */
    int32_t has_key;                /* 0 or 1; 1 only with types 0 (key[0]) and 2 (key[0..2]) */
    uint16_t key[3];
    uint8_t palette[256][4];        /* RGBA, read for type 3 only */
} dvs_png_desc;

/* host only: the value of DVS_PNG_BAND the library was built with */
int dvs_png_band_rows(void);

/* host only: bytes of the filtered stream, height * (1 + rowbytes); 0 for a desc dvs_png_reconstruct refuses */
size_t dvs_png_filtered_bytes(const dvs_png_desc* desc);

/* rgb (and alpha) = the image of `filtered`. `desc` is a HOST pointer, read before the call returns; `filtered` is a DEVICE pointer to
 * dvs_png_filtered_bytes(desc) bytes with no alignment requirement, OVERWRITTEN with the unfiltered scanlines (no scratch buffer is
 * needed); `rgb` is a DEVICE pointer to planar [3][height][width] bytes, the layout dvs_jpeg_reconstruct writes; `alpha` is a nullable
 * DEVICE pointer to [height][width] bytes; neither may overlap `filtered`. The same rgb with or without alpha.
 * DVS_ERR_INVALID for a NULL desc, filtered or rgb, an illegal type / depth pair, or a desc that contradicts itself (a side outside
 * 1..65500, has_key outside {0, 1} or set beside an alpha channel or a palette). */
int dvs_png_reconstruct(void* stream, const dvs_png_desc* desc, uint8_t* filtered, uint8_t* rgb, uint8_t* alpha);

/* ---- PNG encoding: fp32 planes (what dvs_raster_forward_views and dvs_raster_depth_views write) -> filtered scanlines, the mirror image
 * of the above; gstrain/png_io.hpp (write_png) deflates them on the host. One launch takes up to DVS_PNG_ENCODE_MAX_VIEWS views of one
 * size and kind. No scratch; a view's output does not depend on the other views of the call, and two calls return identical bytes and
 * counts. The result is defined bit for bit; after the first step it is integer arithmetic; tests/png_enc_ref.py restates it:
 *   sample       M = 255 (RGB8, GRAY8) or 65535 (GRAY16); s = (int)min(M, max(0, rint(x * scale))): the fp32 product rounded to the
 *                nearest integer, ties to even; NaN -> 0, +inf -> M, -inf -> 0. With scale = 255 this is dvs_jpeg_encode_views' float to
 *                byte rule (PackF32ToU8): a PNG and a JPEG of one render are quantised alike. A sample counts as SATURATED iff
 *                rint(x * scale) > M before the clamp: +inf counts, a NaN does not.
 *   raw scanline RGB8: R G B per pixel, interleaved; GRAY8: one byte per pixel; GRAY16: two, the high byte first
 *   filters      x = the raw byte, a = the raw byte bpp to the left, b = the raw byte above, c = the raw byte above a (as the decoder's
 *                comment above defines them); bytes left of the row and the row above the first read as 0; every difference is taken
 *                modulo 256:   0 None x | 1 Sub x - a | 2 Up x - b | 3 Average x - ((a + b) >> 1) | 4 Paeth x - predictor, the
 *                predictor with the decoder's own tie order (a if pa <= pb and pa <= pc, else b if pb <= pc, else c)
 *   choice       the cost of filter f on a row = the sum over its rowbytes filtered bytes v of (v < 128 ? v : 256 - v), the "minimum sum
 *                of absolute differences" heuristic; an int32 (at most 196 500 * 128). The row gets the filter of the smallest cost, on
 *                a tie the smallest f: a row of zeros gets 0.
 *   output row   the filter byte, then the row filtered with it; rows follow one another at y * (1 + rowbytes) */
#define DVS_PNG_ENCODE_MAX_VIEWS 16
#define DVS_PNG_KIND_RGB8   0   /* images[v]: planar [3][H][W] fp32 -> colour type 2, depth 8  (rowbytes 3W, bpp 3) */
#define DVS_PNG_KIND_GRAY8  1   /* images[v]: [H][W] fp32          -> colour type 0, depth 8  (rowbytes  W, bpp 1) */
#define DVS_PNG_KIND_GRAY16 2   /* images[v]: [H][W] fp32          -> colour type 0, depth 16 (rowbytes 2W, bpp 2, big-endian) */

/* host only: bytes of one view's filtered stream, height * (1 + rowbytes); 0 for a kind or size dvs_png_encode_views refuses */
size_t dvs_png_encode_bytes(int kind, int width, int height);

/* filtered[v] = the filtered stream of images[v], v < n_views, in the layout dvs_png_reconstruct reads. `images` and `filtered` are HOST
 * arrays of DEVICE pointers, read before the call returns; images[v] needs a float's alignment only; filtered[v] points to
 * dvs_png_encode_bytes(kind, width, height) bytes with no alignment requirement: where a lane's four bytes fall on a dword of the
 * output they leave as one dword store, as single bytes otherwise, the same bytes either way. `saturated`: nullable DEVICE
 * uint32[n_views], INCREMENTED by the number of saturated samples of each view (the caller zeroes it; one atomic per wavefront that
 * has any — an integer sum, so the count does not depend on their order).
 * DVS_ERR_INVALID, before anything touches the device, for a NULL images / filtered / images[v] / filtered[v], n_views outside 1..16,
 * an unknown kind, a side outside 1..65500, a scale that is not finite or not > 0, an images[v] off a 4-byte boundary. */
int dvs_png_encode_views(void* stream, int kind, int width, int height, float scale, const float* const* images,
                         uint8_t* const* filtered, uint32_t* saturated, int n_views);

/* ---- the mask rule on the device, so that decoded pixels never travel back to the host: m[i] = gray[i] > 127, AND alpha[i] > 127 when
 * alpha is given, AND other[i] != 0 when other is given (a plane of bytes in {0, 1}, such as an earlier result); written as bytes in
 * {0, 1} to out_u8 and as 0.0f / 1.0f to out_f32, whichever of the two is not NULL (the loader feeds the bytes to dvs_undistort_view
 * and keeps the floats as the view's mask). With gray NULL and other given the call is the converter of a {0, 1} plane to those floats.
 * All pointers are DEVICE pointers to n elements; out_u8 may be one of the inputs (element i is read before it is written).
 * DVS_ERR_INVALID for gray and other both NULL, both outputs NULL, n = 0. */
int dvs_mask_combine(void* stream, size_t n, const uint8_t* gray, const uint8_t* alpha, const uint8_t* other, uint8_t* out_u8, float* out_f32);

#ifdef __cplusplus
}
#endif
#endif
