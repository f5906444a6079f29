// transform.hip — export in a chosen frame (include/dvs_export.h, last section): the model under a similarity p' = s R p + t, for gfx950.
//   host   dvs_similarity_from_trs / dvs_similarity_inverse / dvs_sh_rotation: pure fp64 functions, rounded once to fp32.
//          The SH band matrices are solved by projection: with Y the band's basis (dvs_sh_basis restated in fp64, the fp32 constants of
//          dvs_device.h as they are) at SAMPLES fixed directions d and Y' the same at R d, D = (Y'^T Y')^-1 Y'^T Y — the least-squares
//          solution of Y' D = Y, whose residual is zero because a rotated band function lies in the band's own span.
//   k_transform_splats   a streaming pass over 232 B per splat in and out. One wavefront per 64-splat tile of DVS_SHN_TILED, 256-lane
//          workgroups: a lane loads its splat's twelve 16-byte chunks (the wave moves 1 KiB of contiguous memory per instruction, as
//          k_pack_spz does), rotates the bands in registers and stores twelve chunks. The similarity, the quaternion of R and the 83
//          matrix floats are ONE by-value kernel argument: wave-uniform, read through the kernarg segment into scalar registers, every
//          index a compile-time constant. No LDS, no atomics, no inline assembly. The pointers are NOT __restrict__: in place is allowed.
//          DVS_SHN_ROWS (the interop layout) goes through the same arithmetic with dvs_shn_index addressing.
//   k_transform_points   one thread per mesh vertex.
// Results are defined operation by operation (tests/transform_ref.py restates them in numpy): compiled without contraction (EXACT).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "dvs_device.h"
#include "export_common.h"
#include "../../include/dvs_raster.h"
#include "../../include/dvs_export.h"

namespace {
constexpr int TF_BLOCK = 256, TF_WAVES = TF_BLOCK / 64;

// what the kernels read through the kernarg segment
struct TfArgs {
    float R[9], t[3], s, ls;    // ls = (float)log((double)s)
    float a[4];                 // the unit quaternion of R, (w, x, y, z)
    float D[83];
};

__device__ __forceinline__ float tf_row(const float* r, float x, float y, float z) { return (r[0] * x + r[1] * y) + r[2] * z; }

// one band of M = 2 l + 1 coefficients starting at coefficient FIRST, matrix at D + OFF: out element (FIRST + j) * 3 + c
template <int M, int FIRST, int OFF>
__device__ __forceinline__ void tf_band(const TfArgs& A, const float (&v)[48], float (&o)[48]) {
#pragma unroll
    for (int j = 0; j < M; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float acc = A.D[OFF + j * M] * v[FIRST * 3 + c];
#pragma unroll
            for (int k = 1; k < M; ++k) acc = acc + A.D[OFF + j * M + k] * v[(FIRST + k) * 3 + c];
            o[(FIRST + j) * 3 + c] = acc;
        }
}
// the 45 floats of a splat (v[45..47]: the pads) -> o; bands above `degree` are copied, the pads are 0
__device__ __forceinline__ void tf_rotate_sh(const TfArgs& A, int degree, const float (&v)[48], float (&o)[48]) {
#pragma unroll
    for (int e = 0; e < 45; ++e) o[e] = v[e];
    o[45] = o[46] = o[47] = 0.0f;
    if (degree >= 1) tf_band<3, 0, 0>(A, v, o);
    if (degree >= 2) tf_band<5, 3, 9>(A, v, o);
    if (degree >= 3) tf_band<7, 8, 34>(A, v, o);
}

__global__ void __launch_bounds__(TF_BLOCK)
k_transform_splats(TfArgs A, int n, int degree, int tiled, const float* pos, const float* shN, const float* scale, const float* rot,
                   float* pos_out, float* shN_out, float* scale_out, float* rot_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * TF_WAVES + wave, i = tile * 64 + lane;
    if (tile * 64 >= n) return;                                            // a wave past the model
    const bool valid = i < n;
    if (valid) {
        const float x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
        const float s0 = scale[3 * i], s1 = scale[3 * i + 1], s2 = scale[3 * i + 2];
        const float4 q = reinterpret_cast<const float4*>(rot)[i];        // (w, x, y, z)
        float p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = tf_row(A.R + 3 * k, x, y, z) * A.s + A.t[k];
        pos_out[3 * i] = p[0]; pos_out[3 * i + 1] = p[1]; pos_out[3 * i + 2] = p[2];
        scale_out[3 * i] = s0 + A.ls; scale_out[3 * i + 1] = s1 + A.ls; scale_out[3 * i + 2] = s2 + A.ls;
        float4 r;
        r.x = ((A.a[0] * q.x - A.a[1] * q.y) - A.a[2] * q.z) - A.a[3] * q.w;
        r.y = ((A.a[0] * q.y + A.a[1] * q.x) + A.a[2] * q.w) - A.a[3] * q.z;
        r.z = ((A.a[0] * q.z - A.a[1] * q.w) + A.a[2] * q.x) + A.a[3] * q.y;
        r.w = ((A.a[0] * q.w + A.a[1] * q.z) - A.a[2] * q.y) + A.a[3] * q.x;
        reinterpret_cast<float4*>(rot_out)[i] = r;
    }
    if (!shN) return;                                                      // (degree 0 without the higher bands)
    float v[48], o[48];
    if (tiled) {                                                           // whole tiles are allocated: every lane's chunk is in bounds
#pragma unroll
        for (int c = 0; c < 12; ++c) {
            const float4 w = reinterpret_cast<const float4*>(shN)[dvs_shn_tiled_chunk(i, c)];
            v[4 * c] = w.x; v[4 * c + 1] = w.y; v[4 * c + 2] = w.z; v[4 * c + 3] = w.w;
        }
        tf_rotate_sh(A, degree, v, o);
#pragma unroll
        for (int c = 0; c < 12; ++c)                                       // the lanes past the model write zeros
            reinterpret_cast<float4*>(shN_out)[dvs_shn_tiled_chunk(i, c)] =
                valid ? make_float4(o[4 * c], o[4 * c + 1], o[4 * c + 2], o[4 * c + 3]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    } else if (valid) {
#pragma unroll
        for (int e = 0; e < 45; ++e) v[e] = shN[i * 45 + e];
        v[45] = v[46] = v[47] = 0.0f;
        tf_rotate_sh(A, degree, v, o);
#pragma unroll
        for (int e = 0; e < 45; ++e) shN_out[i * 45 + e] = o[e];
    }
}

__global__ void __launch_bounds__(TF_BLOCK)
k_transform_points(TfArgs A, int n, const float* xyz, const float* normals, float* xyz_out, float* normals_out) {
    const int64_t i = (int64_t)blockIdx.x * TF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    float p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = tf_row(A.R + 3 * k, x, y, z) * A.s + A.t[k];
    xyz_out[3 * i] = p[0]; xyz_out[3 * i + 1] = p[1]; xyz_out[3 * i + 2] = p[2];
    if (!normals) return;
    const float nx = normals[3 * i], ny = normals[3 * i + 1], nz = normals[3 * i + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = tf_row(A.R + 3 * k, nx, ny, nz);
    normals_out[3 * i] = p[0]; normals_out[3 * i + 1] = p[1]; normals_out[3 * i + 2] = p[2];
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
bool tf_rotation_ok(const float R[9]) {
    for (int k = 0; k < 9; ++k) if (!std::isfinite(R[k])) return false;
    double worst = 0.0;                                                     // the infinity norm of R R^T - I: its largest absolute row sum
    for (int r = 0; r < 3; ++r) {
        double row = 0.0;
        for (int c = 0; c < 3; ++c) {
            double d = r == c ? -1.0 : 0.0;
            for (int k = 0; k < 3; ++k) d += (double)R[3 * r + k] * (double)R[3 * c + k];
            row += std::fabs(d);
        }
        worst = std::fmax(worst, row);
    }
    const double det = (double)R[0] * ((double)R[4] * R[8] - (double)R[5] * R[7]) - (double)R[1] * ((double)R[3] * R[8] - (double)R[5] * R[6]) +
                       (double)R[2] * ((double)R[3] * R[7] - (double)R[4] * R[6]);
    return worst <= 1e-4 && det >= 0.0;
}
bool tf_similarity_ok(const dvs_similarity* m) {
    if (!m || !tf_rotation_ok(m->R) || !std::isfinite(m->s) || !(m->s > 0.0f)) return false;
    for (int k = 0; k < 3; ++k) if (!std::isfinite(m->t[k])) return false;
    return true;
}

// the unit quaternion (w, x, y, z) of a rotation matrix, in fp64: the branch of the largest of trace, R00, R11, R22 (the first of equal
// ones in that order), every operation an IEEE addition, multiplication, division or square root (tests/transform_ref.py quat_of_rotation)
void tf_quat_of(const float Rf[9], double q[4]) {
    double R[9];
    for (int k = 0; k < 9; ++k) R[k] = (double)Rf[k];
    const double tr = (R[0] + R[4]) + R[8];
    if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
        const double S = std::sqrt(tr + 1.0) * 2.0;
        q[0] = 0.25 * S; q[1] = (R[7] - R[5]) / S; q[2] = (R[2] - R[6]) / S; q[3] = (R[3] - R[1]) / S;
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        const double S = std::sqrt(((1.0 + R[0]) - R[4]) - R[8]) * 2.0;
        q[0] = (R[7] - R[5]) / S; q[1] = 0.25 * S; q[2] = (R[1] + R[3]) / S; q[3] = (R[2] + R[6]) / S;
    } else if (R[4] >= R[8]) {
        const double S = std::sqrt(((1.0 + R[4]) - R[0]) - R[8]) * 2.0;
        q[0] = (R[2] - R[6]) / S; q[1] = (R[1] + R[3]) / S; q[2] = 0.25 * S; q[3] = (R[5] + R[7]) / S;
    } else {
        const double S = std::sqrt(((1.0 + R[8]) - R[0]) - R[4]) * 2.0;
        q[0] = (R[3] - R[1]) / S; q[1] = (R[2] + R[6]) / S; q[2] = (R[5] + R[7]) / S; q[3] = 0.25 * S;
    }
    const double len = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);      // (R is a rotation to 1e-4 only)
    for (int k = 0; k < 4; ++k) q[k] = q[k] / len;
}

TfArgs tf_args(const dvs_similarity& m, const float* D) {
    TfArgs A{};
    for (int k = 0; k < 9; ++k) A.R[k] = m.R[k];
    for (int k = 0; k < 3; ++k) A.t[k] = m.t[k];
    A.s = m.s;
    A.ls = (float)std::log((double)m.s);
    double q[4];
    tf_quat_of(m.R, q);
    for (int k = 0; k < 4; ++k) A.a[k] = (float)q[k];
    if (D) for (int k = 0; k < 83; ++k) A.D[k] = D[k];
    return A;
}

// dvs_sh_basis in fp64, the constants as the kernels have them (fp32 values); b[0..15) = the coefficients 0..14 above the dc term
void tf_basis(double x, double y, double z, double b[15]) {
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    b[0] = -(double)DVS_SH_C1 * y; b[1] = (double)DVS_SH_C1 * z; b[2] = -(double)DVS_SH_C1 * x;
    b[3] = (double)DVS_SH_C2_0 * xy;
    b[4] = (double)DVS_SH_C2_1 * yz;
    b[5] = (double)DVS_SH_C2_2 * (2.0 * zz - xx - yy);
    b[6] = (double)DVS_SH_C2_3 * xz;
    b[7] = (double)DVS_SH_C2_4 * (xx - yy);
    b[8] = (double)DVS_SH_C3_0 * y * (3.0 * xx - yy);
    b[9] = (double)DVS_SH_C3_1 * xy * z;
    b[10] = (double)DVS_SH_C3_2 * y * (4.0 * zz - xx - yy);
    b[11] = (double)DVS_SH_C3_3 * z * (2.0 * zz - 3.0 * xx - 3.0 * yy);
    b[12] = (double)DVS_SH_C3_4 * x * (4.0 * zz - xx - yy);
    b[13] = (double)DVS_SH_C3_5 * z * (xx - yy);
    b[14] = (double)DVS_SH_C3_6 * x * (xx - 3.0 * yy);
}

// solves G X = B in place (G m x m, B m x m, row-major with stride 7): Gaussian elimination with partial pivoting
bool tf_solve(int m, double G[7][7], double B[7][7]) {
    for (int c = 0; c < m; ++c) {
        int piv = c;
        for (int r = c + 1; r < m; ++r) if (std::fabs(G[r][c]) > std::fabs(G[piv][c])) piv = r;
        if (!(std::fabs(G[piv][c]) > 1e-12)) return false;
        if (piv != c) for (int k = 0; k < m; ++k) { std::swap(G[piv][k], G[c][k]); std::swap(B[piv][k], B[c][k]); }
        for (int r = 0; r < m; ++r) {
            if (r == c) continue;
            const double f = G[r][c] / G[c][c];
            if (f == 0.0) continue;
            for (int k = 0; k < m; ++k) { G[r][k] -= f * G[c][k]; B[r][k] -= f * B[c][k]; }
        }
    }
    for (int r = 0; r < m; ++r) for (int k = 0; k < m; ++k) B[r][k] /= G[r][r];
    return true;
}
}  // namespace

extern "C" int dvs_similarity_from_trs(const float t[3], const float euler_rad[3], float s, dvs_similarity* out) {
    if (!t || !euler_rad || !out || !std::isfinite(s) || !(s > 0.0f)) return DVS_ERR_INVALID;
    for (int k = 0; k < 3; ++k) if (!std::isfinite(t[k]) || !std::isfinite(euler_rad[k])) return DVS_ERR_INVALID;
    // R = Rz Ry Rx through the half-angle quaternion, as dvs_region_from_trs forms it (region.hip)
    const double cx = std::cos(0.5 * (double)euler_rad[0]), sx = std::sin(0.5 * (double)euler_rad[0]), cy = std::cos(0.5 * (double)euler_rad[1]),
                 sy = std::sin(0.5 * (double)euler_rad[1]), cz = std::cos(0.5 * (double)euler_rad[2]), sz = std::sin(0.5 * (double)euler_rad[2]);
    const double w = cx * cy * cz + sx * sy * sz, x = sx * cy * cz - cx * sy * sz, y = cx * sy * cz + sx * cy * sz, z = cx * cy * sz - sx * sy * cz;
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    for (int k = 0; k < 9; ++k) out->R[k] = (float)R[k];
    for (int k = 0; k < 3; ++k) out->t[k] = t[k];
    out->s = s;
    return DVS_OK;
}

extern "C" int dvs_similarity_inverse(const dvs_similarity* in, dvs_similarity* out) {
    if (!out || !tf_similarity_ok(in)) return DVS_ERR_INVALID;
    dvs_similarity r;
    for (int k = 0; k < 3; ++k) {
        double acc = 0.0;
        for (int c = 0; c < 3; ++c) { r.R[3 * k + c] = in->R[3 * c + k]; acc += (double)in->R[3 * c + k] * (double)in->t[c]; }
        r.t[k] = (float)(-acc / (double)in->s);
    }
    r.s = (float)(1.0 / (double)in->s);
    if (!std::isfinite(r.s) || !(r.s > 0.0f)) return DVS_ERR_INVALID;     // (an s whose reciprocal is not an fp32 number)
    *out = r;
    return DVS_OK;
}

extern "C" int dvs_sh_rotation(const float R[9], float D[83]) {
    if (!R || !D || !tf_rotation_ok(R)) return DVS_ERR_INVALID;
    constexpr int SAMPLES = 96;
    static const int first[3] = {0, 3, 8}, size[3] = {3, 5, 7}, off[3] = {0, 9, 34};
    double G[3][7][7] = {}, B[3][7][7] = {};
    for (int k = 0; k < SAMPLES; ++k) {                                     // a Fibonacci spiral: fixed, well spread, no symmetry
        const double z = 1.0 - (2.0 * k + 1.0) / SAMPLES, rad = std::sqrt(1.0 - z * z), phi = 2.399963229728653 * k;
        const double d[3] = {rad * std::cos(phi), rad * std::sin(phi), z};
        double e[3];
        for (int r = 0; r < 3; ++r) e[r] = ((double)R[3 * r] * d[0] + (double)R[3 * r + 1] * d[1]) + (double)R[3 * r + 2] * d[2];
        double y0[15], y1[15];
        tf_basis(d[0], d[1], d[2], y0);
        tf_basis(e[0], e[1], e[2], y1);
        for (int l = 0; l < 3; ++l)
            for (int a = 0; a < size[l]; ++a)
                for (int b = 0; b < size[l]; ++b) {
                    G[l][a][b] += y1[first[l] + a] * y1[first[l] + b];
                    B[l][a][b] += y1[first[l] + a] * y0[first[l] + b];
                }
    }
    float out[83];
    for (int l = 0; l < 3; ++l) {
        if (!tf_solve(size[l], G[l], B[l])) return DVS_ERR_INVALID;
        // (an entry below 1e-14 is below the solve's own error: an exact 0, so that the identity and the axis turns give exact matrices)
        for (int a = 0; a < size[l]; ++a)
            for (int b = 0; b < size[l]; ++b) out[off[l] + a * size[l] + b] = std::fabs(B[l][a][b]) < 1e-14 ? 0.0f : (float)B[l][a][b];
    }
    for (int k = 0; k < 83; ++k) D[k] = out[k];
    return DVS_OK;
}

extern "C" int dvs_transform_splats(void* stream, int n, int sh_degree, const dvs_similarity* sim, const float* D, const float* pos,
                                    const float* shN, int shn_layout, const float* scale, const float* rot, float* pos_out, float* shN_out,
                                    float* scale_out, float* rot_out) {
    if (n <= 0 || sh_degree < 0 || sh_degree > 3 || !D || !tf_similarity_ok(sim) || ((!shN || !shN_out) && sh_degree > 0) ||
        dvs_bad_args({pos, scale, rot, pos_out, scale_out, rot_out}, {shN, shN_out}, shn_layout))
        return DVS_ERR_INVALID;
    for (int k = 0; k < 83; ++k) if (!std::isfinite(D[k])) return DVS_ERR_INVALID;
    const bool sh = shN && shN_out;
    const TfArgs A = tf_args(*sim, D);
    const unsigned nblocks = (unsigned)(((int64_t)n + TF_BLOCK - 1) / TF_BLOCK);
    hipLaunchKernelGGL(k_transform_splats, dim3(nblocks), dim3(TF_BLOCK), 0, (hipStream_t)stream, A, n, sh_degree, shn_layout == DVS_SHN_TILED ? 1 : 0,
                       pos, sh ? shN : nullptr, scale, rot, pos_out, sh ? shN_out : nullptr, scale_out, rot_out);
    return dvs_launch_status();
}

extern "C" int dvs_transform_points(void* stream, int n, const dvs_similarity* sim, const float* xyz, const float* normals, float* xyz_out,
                                    float* normals_out) {
    if (n <= 0 || !tf_similarity_ok(sim) || !xyz || !xyz_out || (normals && !normals_out)) return DVS_ERR_INVALID;
    const TfArgs A = tf_args(*sim, nullptr);
    const unsigned nblocks = (unsigned)(((int64_t)n + TF_BLOCK - 1) / TF_BLOCK);
    hipLaunchKernelGGL(k_transform_points, dim3(nblocks), dim3(TF_BLOCK), 0, (hipStream_t)stream, A, n, xyz, normals, xyz_out, normals_out);
    return dvs_launch_status();
}
