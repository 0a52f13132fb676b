// Sanitizer harness for the bias split of an L2 store: vod_amd/csrc/kernels_l2.hip (its host side: vodhip_debug_l2_split) and
// vod_amd/csrc/l2_bias.h compiled as HOST C++ with -fsanitize=address,undefined.  Sweeps c = -|x|^2 / 2 over every half-integer up to
// 2^16, powers of two and their neighbours, random magnitudes and values around and beyond the limit, for both store dtypes, and checks
// in double precision that the three terms times the three constants give c back within the stated residual, that no term is
// subnormal, and that saturation is reported.  Built and run by tests/test_l2_sanitize_cpu.py; nothing here touches a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "vodhip.h"

namespace {

double term_value(uint16_t b, int dtype) {
    if (dtype == VODHIP_BF16) {
        const uint32_t u = (uint32_t)b << 16;
        float f;
        memcpy(&f, &u, 4);
        return f;
    }
    const int sign = b >> 15, e = (b >> 10) & 31, m = b & 1023;
    double v = e == 0 ? std::ldexp((double)m, -24) : (e == 31 ? INFINITY : std::ldexp(1.0 + m / 1024.0, e - 15));
    return sign ? -v : v;
}

bool subnormal(uint16_t b, int dtype) {
    return dtype == VODHIP_F16 ? ((b & 0x7C00) == 0 && (b & 0x03FF) != 0) : ((b & 0x7F80) == 0 && (b & 0x007F) != 0);
}

long g_errors = 0, g_checked = 0;

void check(float c, int dtype) {
    uint16_t t[3];
    float a[3];
    const int sat = vodhip_debug_l2_split(c, dtype, t, a);
    const double limit = dtype == VODHIP_F16 ? 65504.0 * 256.0 : std::ldexp(1.0, 120);
    const double residual = dtype == VODHIP_F16 ? std::ldexp(1.0, -28) : std::ldexp(1.0, -126);
    double sum = 0.0;
    bool bad = sat < 0;
    for (int i = 0; i < 3; ++i) {
        sum += (double)a[i] * term_value(t[i], dtype);
        bad = bad || subnormal(t[i], dtype);
    }
    const bool beyond = !(std::fabs((double)c) <= limit);  // (also NaN)
    if (beyond) bad = bad || sat != 1 || sum != -limit;
    else bad = bad || sat != 0 || std::fabs(sum - (double)c) > residual;
    if (!beyond && std::fabs((double)c) < 2097152.0 && 2.0 * c == std::nearbyint(2.0 * c)) bad = bad || sum != (double)c;
    ++g_checked;
    if (bad && ++g_errors <= 10) std::printf("c=%.9g dtype=%d: sat=%d sum=%.17g\n", c, dtype, sat, sum);
}

}  // namespace

int main() {
    std::mt19937_64 rng(20260219);
    std::uniform_real_distribution<double> expo(-40.0, 26.0);
    for (int dtype = VODHIP_F16; dtype <= VODHIP_BF16; ++dtype) {
        for (int h = 0; h <= (1 << 17); ++h) check(-0.5f * (float)h, dtype);
        for (int e = -60; e <= 126; ++e) {
            const float p = std::ldexp(1.0f, e);
            check(-p, dtype);
            check(-std::nextafter(p, 0.0f), dtype);
            check(-std::nextafter(p, INFINITY), dtype);
        }
        for (int i = 0; i < 200000; ++i) check(-(float)std::exp2(expo(rng)), dtype);
        const float special[] = {-16769024.f, -16769026.f, -3.0e38f, -INFINITY, NAN, 0.f, -0.f, 1.0f, 12345.5f};
        for (float c : special) check(c, dtype);
    }
    uint16_t t[3];
    float a[3];
    if (vodhip_debug_l2_split(-1.f, VODHIP_F32, t, a) != -1 || vodhip_debug_l2_split(-1.f, VODHIP_F16, nullptr, a) != -1) ++g_errors;
    std::printf("%ld values checked, %ld errors\n", g_checked, g_errors);
    return g_errors ? 1 : 0;
}
