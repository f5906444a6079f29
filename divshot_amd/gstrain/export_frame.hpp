// export_frame.hpp — the export frame's host side (INTEGRATION.md "Export frame"): which rotation and translation turn a capture
// upright and centre it, from its training cameras alone. Pure functions in fp64: no device, no statics, no files.
#pragma once
#include <cstddef>
#include <string>

namespace gsframe {
// "+x" "-x" "+y" "-y" "+z" "-z" -> the unit axis; false for anything else
bool parse_axis(const char* s, double axis[3]);

// p' = R p + t (s = 1) such that
//   R  is the shortest-arc rotation taking u, the normalised mean of the cameras' world-space image-up vectors, onto `axis`. A camera
//      looks along +z with y DOWN (COLMAP's convention, dvs_make_camera_intrinsics), so its image-up vector in world space is minus
//      the second row of its world-to-camera rotation: -(view[1], view[5], view[9]) of dvs_camera.view (view[c * 4 + r]).
//      u exactly opposite to axis (1 + u . axis < 1e-12): the half turn about the coordinate axis that follows the target's cyclically
//      (x -> y, y -> z, z -> x).
//   t  = -R c, c the centroid of the camera centres: it moves to the origin.
// views [n][16], centres [n][3]. R row-major; up (nullable) receives u. false with *err: no camera, a non-finite input, or a mean up
// vector shorter than 1e-6 (the cameras' up vectors cancel: there is no preferred direction).
bool orientation(size_t n, const float* views, const float* centres, const double axis[3], double R[9], double t[3], double up[3], std::string* err);
}  // namespace gsframe
