// The galaxy entry's keep decision on the CPU: quad_rows_and_meet (k_render.h) against the test it stands in for,
// 0.5 * quad_min_rect(...) <= Tk, on random and on edge-placed (component, rectangle) pairs.  The two functions are the
// kernel's own text: tests/test_setup_rules.py cuts the span between k_render.h's "host-checked" marks into quad_rules.inc.
// rcp_f32 / sqrt_f32 are correctly rounded here (the device's are within 1 ulp: inside what the "too close" band allows for).
//
// Claims, per pair:  +1 => the old test keeps;  0 => the old test drops;  -1 (the kernel then runs the old test) is rare.
// So the kernel's decision is the old test's for every pair, and the count of decisions that differ is 0 by construction
// of the -1 branch; what can fail here is a SURE answer that the old test contradicts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define __device__
#define __forceinline__ inline
static inline float rcp_f32(float x) { return (float)(1.0 / (double)x); }
static inline float sqrt_f32(float x) { return (float)std::sqrt((double)x); }
using std::fmax;
using std::fmin;
#include "quad_rules.inc"

static uint64_t s_state = 0x9e3779b97f4a7c15ull;
static double uni() {   // xorshift64*: the same pairs on every run
    s_state ^= s_state >> 12; s_state ^= s_state << 25; s_state ^= s_state >> 27;
    return (double)((s_state * 0x2545f4914f6cdd1dull) >> 11) * (1.0 / 9007199254740992.0);
}
static double uni(double lo, double hi) { return lo + (hi - lo) * uni(); }
static double logu(double lo, double hi) { return std::exp(uni(std::log(lo), std::log(hi))); }

int main(int argc, char **argv) {
    const long n = argc > 1 ? std::atol(argv[1]) : 1000000;
    long sure_keep = 0, sure_drop = 0, close = 0, close_random = 0, old_keep = 0, wrong = 0, placed = 0;
    double worst_sure = INFINITY;     // smallest |0.5 qmin - Tk| among the sure answers
    for (long i = 0; i < n; i++) {
        // covariance: the benchmark's components run from a sharp PSF core (0.1 pixel) to the outer de Vaucouleurs term of a
        // large galaxy (30 pixels), axis ratios down to 0.1, any angle; Tk = T + log(A / eps) from below zero to 60
        const double s1 = logu(0.1, 30.0), s2 = s1 * uni(0.1, 1.0), th = uni(0.0, M_PI);
        const double cs = std::cos(th), sn = std::sin(th);
        const double cxx = s1 * s1 * cs * cs + s2 * s2 * sn * sn, cyy = s1 * s1 * sn * sn + s2 * s2 * cs * cs,
                     cxy = (s1 * s1 - s2 * s2) * cs * sn;
        const double det = cxx * cyy - cxy * cxy;
        const double a = cyy / det, b = -cxy / det, c = cxx / det;
        const double dq = a * c - b * b;      // the FORM's determinant (1 / det): what the ellipse's ends are made of
        const double Tk = uni(-5.0, 60.0), R = 2.0 * fmax(Tk, 0.0);
        // the rectangle: 1..32 columns, 1..64 rows, integer coordinates about a fractional centre up to four radii away
        const double reach = 4.0 * s1 * std::sqrt(fmax(R, 1.0)) + 8.0;
        const double mx = uni(0.0, 1.0), my = uni(0.0, 1.0);
        const int w = 1 + (int)(uni() * 32.0), h = 1 + (int)(uni() * 64.0);
        double x1 = std::floor(uni(-reach, reach)) - mx, y1 = std::floor(uni(-reach, reach)) - my;
        const bool place = (R > 0.0 && (i & 1));
        if (place) {
            // every second pair: an edge of the rectangle PLACED on the ellipse's end, 1e-7 .. 1e-1 to either side of it --
            // a row end (the y-interval of the ellipse over the rectangle's columns), or the x-extent (the flank)
            placed++;
            const double off = (uni() < 0.5 ? -1.0 : 1.0) * logu(1e-7, 1e-1);
            const int which = (int)(uni() * 4.0);
            if (which >= 2) {
                const double X = std::sqrt(c * R / dq);
                x1 = (which == 2) ? X + off : -X + off - (double)(w - 1);
            } else {
                // ends of the exact interval over [x1, x1 + w - 1]
                const double xs = b * std::sqrt(R / (dq * a)), x2 = x1 + (double)(w - 1);
                const double xt = fmin(fmax(-xs, x1), x2), xb = fmin(fmax(xs, x1), x2);
                const double at = c * R - dq * xt * xt, ab = c * R - dq * xb * xb;
                if (at > 0.0 && ab > 0.0) {
                    const double yhi = (-b * xt + std::sqrt(at)) / c, ylo = (-b * xb - std::sqrt(ab)) / c;
                    y1 = (which == 0) ? yhi + off : ylo + off - (double)(h - 1);
                }
            }
        }
        const double x2 = x1 + (double)(w - 1), y2 = y1 + (double)(h - 1);
        const double half_qmin = 0.5 * quad_min_rect(a, b, c, x1, x2, y1, y2);
        const bool old = (half_qmin <= Tk);
        float ylo, yhi;
        const int meet = quad_rows_and_meet(a, b, c, Tk, x1, x2, y1, y2, ylo, yhi);
        old_keep += old;
        if (meet < 0) { close++; close_random += !place; continue; }
        (meet ? sure_keep : sure_drop)++;
        worst_sure = fmin(worst_sure, std::fabs(half_qmin - Tk));
        if ((meet > 0) != old) {
            if (wrong++ < 10)
                std::printf("WRONG: meet %d old %d  a %.17g b %.17g c %.17g R %.17g rect [%.17g, %.17g] x [%.17g, %.17g] 0.5 qmin - Tk %.3g\n",
                            meet, (int)old, a, b, c, R, x1, x2, y1, y2, half_qmin - Tk);
        }
    }
    std::printf("pairs %ld (edge-placed %ld): old test keeps %ld; sure keep %ld, sure drop %ld, too close %ld (of the random pairs %ld); "
                "sure answers the old test contradicts %ld; nearest sure answer |0.5 qmin - Tk| %.3g\n",
                n, placed, old_keep, sure_keep, sure_drop, close, close_random, wrong, worst_sure);
    return wrong ? 1 : 0;
}
