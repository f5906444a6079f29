// export_frame.cpp — see export_frame.hpp. Also the plain-C entry point libgsplyio.so exports for the CPU tests.
#include "export_frame.hpp"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

namespace gsframe {
bool parse_axis(const char* s, double axis[3]) {
    if (!s || strlen(s) != 2 || (s[0] != '+' && s[0] != '-') || s[1] < 'x' || s[1] > 'z') return false;
    axis[0] = axis[1] = axis[2] = 0.0;
    axis[s[1] - 'x'] = s[0] == '+' ? 1.0 : -1.0;
    return true;
}

bool orientation(size_t n, const float* views, const float* centres, const double axis[3], double R[9], double t[3], double up[3], std::string* err) {
    const auto fail = [&](const char* why) { if (err) *err = why; return false; };
    if (n == 0 || !views || !centres) return fail("no training camera");
    double u[3] = {0, 0, 0}, c[3] = {0, 0, 0};
    for (size_t k = 0; k < n; ++k)
        for (int a = 0; a < 3; ++a) {
            const double v = -(double)views[16 * k + 4 * a + 1], p = (double)centres[3 * k + a];
            if (!std::isfinite(v) || !std::isfinite(p)) return fail("a camera that is not finite");
            u[a] += v; c[a] += p;
        }
    for (int a = 0; a < 3; ++a) { u[a] /= (double)n; c[a] /= (double)n; }
    const double len = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    if (!(len >= 1e-6)) return fail("the mean of the cameras' up vectors is shorter than 1e-6: they cancel, no direction to turn upright");
    for (int a = 0; a < 3; ++a) u[a] /= len;
    if (up) for (int a = 0; a < 3; ++a) up[a] = u[a];
    const double d = u[0] * axis[0] + u[1] * axis[1] + u[2] * axis[2];
    if (1.0 + d < 1e-12) {                                                  // opposite: a half turn about the next coordinate axis, R = 2 p p^T - I
        int k = 0;
        for (int a = 0; a < 3; ++a) if (axis[a] != 0.0) k = a;
        double p[3] = {0, 0, 0};
        p[(k + 1) % 3] = 1.0;
        for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) R[3 * r + q] = 2.0 * p[r] * p[q] - (r == q ? 1.0 : 0.0);
    } else {                                                                // R = I + [v]x + [v]x^2 / (1 + d), v = u x axis
        const double v[3] = {u[1] * axis[2] - u[2] * axis[1], u[2] * axis[0] - u[0] * axis[2], u[0] * axis[1] - u[1] * axis[0]};
        const double K[9] = {0, -v[2], v[1], v[2], 0, -v[0], -v[1], v[0], 0};
        const double f = 1.0 / (1.0 + d);
        for (int r = 0; r < 3; ++r)
            for (int q = 0; q < 3; ++q) {
                double k2 = 0.0;
                for (int m = 0; m < 3; ++m) k2 += K[3 * r + m] * K[3 * m + q];
                R[3 * r + q] = (r == q ? 1.0 : 0.0) + K[3 * r + q] + f * k2;
            }
    }
    for (int r = 0; r < 3; ++r) t[r] = -(R[3 * r] * c[0] + R[3 * r + 1] * c[1] + R[3 * r + 2] * c[2]);
    return true;
}
}  // namespace gsframe

#ifdef GSPLYIO_CAPI
// 0: R [9] row-major and t [3] written; 1: refused, the message in err_out (when given, NUL-terminated, at most err_cap bytes)
extern "C" __attribute__((visibility("default"))) int gstrain_export_orientation(uint64_t n, const float* views, const float* centres, const char* axis,
                                                                                  double* R, double* t, char* err_out, uint64_t err_cap) {
    std::string err;
    double a[3];
    bool ok = R && t && gsframe::parse_axis(axis, a);
    if (!ok) err = "the axis is not one of +x -x +y -y +z -z";
    else ok = gsframe::orientation((size_t)n, views, centres, a, R, t, nullptr, &err);
    if (ok) return 0;
    if (err_out && err_cap > 0) { const size_t k = std::min<size_t>(err.size(), (size_t)err_cap - 1); memcpy(err_out, err.data(), k); err_out[k] = 0; }
    return 1;
}
#endif
