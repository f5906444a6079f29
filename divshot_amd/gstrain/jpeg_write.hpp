// jpeg_write.hpp — the serial half of baseline JPEG encoding: quantised DCT coefficients -> a JFIF byte stream, the mirror image of
// jpeg_io.hpp. Host only, no GPU dependency, no library; a pure function without mutable globals or statics, so any number of threads
// may code different frames at once. The parallel half (float -> byte, colour conversion, subsampling, forward DCT, quantisation) is
// dvs_jpeg_encode_views (include/dvs_image.h).
//   Written: SOI, APP0 (JFIF 1.01, no density), one DQT segment per distinct quantiser table (two for a frame of the device's encoder:
//            Y, and Cb = Cr; a frame whose Cb and Cr tables differ gets a third), SOF0, four DHT with the Annex K tables (K.3 - K.6),
//            SOS, ONE interleaved scan (DC differences, ZRL for runs of 16 zeros, EOB, a stuffed 00 after every FF byte, the last
//            byte padded with 1 bits), EOI. No restart markers, no optimised tables.
//   Refused with a message, never a crash: a NULL argument, a frame that contradicts itself (sizes, components other than 1 or 3,
//            sampling other than luma 1x1 / 2x1 / 2x2 with chroma 1x1, block counts that are not the size's, offsets or a coefficient
//            array that do not hold the blocks), a quantiser of 0 or above 255 (a baseline DQT holds bytes), a coefficient outside
//            [-1023, 1023] (the Annex K tables have no code for a larger AC value; a DC value is held to the same range so that every
//            DC difference fits the 11 bits of the largest category).
// decode_coefficients(encode_coefficients(F)) returns F: sizes, sampling, quantisers, every coefficient.
#pragma once
#include <cstdint>
#include <string>
#include "jpeg_io.hpp"

namespace gsjpeg {

// `out` receives the file's bytes (a std::string used as a byte buffer)
bool encode_coefficients(const Frame& frame, std::string* out, std::string* err);
// the same over the pieces of a frame (what crosses a C boundary): coef holds n_coef values
bool encode_coefficients(int width, int height, int components, const int hs[3], const int vs[3], const uint16_t quant[3][64],
                         const int blocks_w[3], const int blocks_h[3], const uint64_t offset[3], const int16_t* coef, uint64_t n_coef,
                         std::string* out, std::string* err);

}  // namespace gsjpeg
