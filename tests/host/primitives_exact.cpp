// The device math primitives against exact references: exp_tab64, exp_tab256_p3, log_tab, rcp64, rsqrt64, rcp_rsqrt (k_render.h),
// fast_rcp and the Philox routines (k_split.h).  The functions are the kernels' own text: tests/test_primitives.py cuts the spans
// between the headers' "prim-checked" marks into prim_common.inc / prim_render.inc / prim_split.inc and compiles this file as
// plain C++ without contraction.  The reference is x87 long double (64-bit mantissa) throughout: never another fp64 routine.
//
//   primitives_exact cpu N            the functions as cut, on the host: N random arguments per function + the edge sets
//   primitives_exact gen DIR N        write the argument files a device run reads (N random per function + the edge sets)
//   primitives_exact check DIR        hold the result files of a device run (tests/device/prim_probe.hip) to the same references
//
// Output: "key value [argument]" lines; the test holds them to the bounds its docstring derives.
// The fp32 instructions are stood in for by the correctly rounded fp32 result moved by g_shift fp32 ulp (-1, 0, +1).
#include <cfloat>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <math.h>
#include <string>
#include <thread>
#include <vector>

#define __device__
#define __forceinline__ inline
static int g_shift = 0;
static inline float shifted(float v) {
    if (g_shift > 0) return nextafterf(v, INFINITY);
    if (g_shift < 0) return nextafterf(v, -INFINITY);
    return v;
}
// (the double quotient rounds to fp32 as the exact one does: 53 >= 2 * 24 + 2; the reciprocal square root is within 2^-28 fp32 ulp of that)
static inline float rcp_f32(float x) { return shifted((float)(1.0 / (double)x)); }
static inline float rsq_f32(float x) { return shifted((float)(1.0 / sqrt((double)x))); }
#include "prim_common.inc"
#include "prim_render.inc"
#include "prim_split.inc"

typedef long double ld;
static const ld LN2L = 0.693147180559945309417232121458176568L;

// ---- helpers -------------------------------------------------------------------------------------------------------------
static uint64_t s_state;
static void seed(uint64_t s) { s_state = s * 0x9e3779b97f4a7c15ull + 0x2545f4914f6cdd1dull; }
static uint64_t u64() { s_state ^= s_state >> 12; s_state ^= s_state << 25; s_state ^= s_state >> 27; return s_state * 0x2545f4914f6cdd1dull; }
static double uni() { return (double)(u64() >> 11) * (1.0 / 9007199254740992.0); }
static double uni(double lo, double hi) { return lo + (hi - lo) * uni(); }
static double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
static uint64_t to_bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }

// one unit in the last place of the fp64 binade that holds the exact value v
static ld ulp_of(ld v) {
    if (v == 0.0L) return 0.0L;
    int e;
    (void)frexpl(fabsl(v), &e);
    if (e - 53 < -1074) e = -1074 + 53;
    return ldexpl(1.0L, e - 53);
}

struct Worst {
    double v = 0.0, at = 0.0;
    void take(double x, double arg) { if (x > v || x != x) { v = x; at = arg; } }
    void merge(const Worst &o) { take(o.v, o.at); }
};
static void say(const char *key, const Worst &w) { printf("%s %.6e %a\n", key, w.v, w.at); }
static void say(const char *key, long v) { printf("%s %ld\n", key, v); }

static int n_threads() {
    unsigned h = std::thread::hardware_concurrency();
    const char *e = getenv("OMP_NUM_THREADS");
    if (e && atoi(e) > 0) h = (unsigned)atoi(e);
    return (int)(h < 1 ? 1 : (h > 16 ? 16 : h));
}
// f(lo, hi, slot) over [0, n) in contiguous pieces, one per thread
static void parallel(size_t n, const std::function<void(size_t, size_t, int)> &f, int T) {
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++) th.emplace_back(f, n * t / T, n * (t + 1) / T, t);
    for (auto &x : th) x.join();
}

static bool read_file(const std::string &p, std::vector<double> &v) {
    FILE *f = fopen(p.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t)sz / 8);
    size_t got = fread(v.data(), 8, v.size(), f);
    fclose(f);
    return got == v.size();
}
static bool write_file(const std::string &p, const std::vector<double> &v) {
    FILE *f = fopen(p.c_str(), "wb");
    if (!f) return false;
    size_t put = fwrite(v.data(), 8, v.size(), f);
    return fclose(f) == 0 && put == v.size();
}

// ---- tables --------------------------------------------------------------------------------------------------------------
struct Tables { double et[64], et256[256], lt[128]; };
static void host_tables(Tables &T) {
    for (int j = 0; j < 64; j++) {
        T.et[j] = (double)exp2l((ld)j / 64.0L);          // correctly rounded but for long double's own last bit (2^-11 ulp)
        exp_tab256_fill(T.et256, j, T.et[j]);              // the kernels' recipe, on that value
    }
    log_tab_fill(T.lt, T.lt + 64);                         // the host's own recipe (device_common.h)
}
// the entries against the exact powers and logarithms
static void check_tables(const Tables &T) {
    Worst e64, e256, ic, lc;
    for (int j = 0; j < 64; j++) {
        const ld x = exp2l((ld)j / 64.0L);
        e64.take((double)(fabsl((ld)T.et[j] - x) / ulp_of(x)), j);
        const ld c = 1.0L + ((ld)j + 0.5L) / 64.0L, r = 1.0L / c;
        ic.take((double)(fabsl((ld)T.lt[j] - r) / ulp_of(r)), j);
        const ld l = -logl((ld)T.lt[j]);                   // of the entry itself: log_tab's identity is about the rounded ic
        lc.take((double)(fabsl((ld)T.lt[64 + j] - l) / ulp_of(l)), j);
    }
    for (int j = 0; j < 256; j++) {
        const ld x = exp2l((ld)j / 256.0L);
        e256.take((double)(fabsl((ld)T.et256[j] - x) / x * 0x1p53L), j);
    }
    say("tab_et64_ulp", e64); say("tab_et256_relu", e256); say("tab_ic_ulp", ic); say("tab_lc_ulp", lc);
}

// ---- arguments -----------------------------------------------------------------------------------------------------------
// exponentials: t in units of ln2 / per (per = 64 or 256)
static void exp_args(std::vector<double> &a, size_t n, int per) {
    seed(per);
    const double sc = (double)((ld)per / LN2L), top = 709.0 * sc;
    a.clear();
    // every table index at several exponents: t = n, n -+ 0.5 (rint's ties) and the fp64 neighbours of each
    const int E[] = {-1009, -1000, -512, -64, -2, -1, 0, 1, 63, 512, 1000, 1022};
    for (int e : E)
        for (int j = 0; j < per; j++)
            for (int h = -1; h <= 1; h++) {
                const double c = (double)e * per + j + 0.5 * h;
                const double v[3] = {nextafter(c, -INFINITY), c, nextafter(c, INFINITY)};
                for (double t : v) if (t <= top && t >= -700.0 * sc) a.push_back(t);
            }
    for (size_t i = 0; i < n; i++) {
        const int k = (int)(u64() % 10);
        double x;
        if (k < 4) x = uni(-700.0, 709.0);                 // the whole range of normal results up to the comment's ceiling
        else if (k < 6) x = uni(-680.0, 680.0);            // REC_EMAX
        else if (k < 8) x = uni(-42.0, 0.0);               // the split's exponent
        else if (k < 9) x = uni(-1.0, 1.0);
        else x = (uni() < 0.5 ? -1.0 : 1.0) * exp(uni(-40.0, 0.0));
        double t = x * sc;
        if (t > top) t = top;
        a.push_back(t);
    }
}
static const double LOG_SPECIAL[] = {0.0, -0.0, -1.0, -INFINITY, INFINITY, NAN, 4.9406564584124654e-324, 2.2250738585072009e-308,
                                     1e-310, -1e-310};
static void log_args(std::vector<double> &a, size_t n) {
    seed(7);
    a.clear();
    const int E[] = {-1022, -1000, -512, -100, -10, -3, -2, -1, 0, 1, 2, 3, 10, 100, 512, 1000, 1023};
    for (int e : E) {
        for (int j = 0; j < 64; j++)                       // every cell: 32 points inside it
            for (int k = 0; k < 32; k++) a.push_back(ldexp(1.0 + (j + uni()) / 64.0, e));
        for (int j = 0; j <= 64; j++) {                    // every cell edge and both neighbours
            const double c = ldexp(1.0 + j / 64.0, e);
            if (e == 1023 && j == 64) continue;
            a.push_back(c); a.push_back(nextafter(c, INFINITY));
            if (!(e == -1022 && j == 0)) a.push_back(nextafter(c, 0.0));
        }
    }
    for (int k = 1; k <= 52; k++) { a.push_back(1.0 + ldexp(1.0, -k)); a.push_back(1.0 - ldexp(1.0, -k)); }
    a.push_back(1.0); a.push_back(nextafter(1.0, 0.0)); a.push_back(nextafter(1.0, 2.0));
    a.push_back(DBL_MAX); a.push_back(DBL_MIN);
    for (size_t i = 0; i < n; i++) {
        const int k = (int)(u64() % 8);
        double x;
        if (k < 3) x = uni(0.5, 2.0);                                           // dense on [0.5, 2)
        else if (k < 5) x = 1.0 + (uni() < 0.5 ? -0.5 : 1.0) * exp(uni(-36.0, 0.0));   // towards 1 from both sides
        else if (k < 6) x = uni(1.0 - 1.0 / 128.0, 1.0 + 1.0 / 64.0);
        else x = from_bits((u64() % 0x7fe0000000000000ull) + 0x0010000000000000ull);    // any normal number
        a.push_back(x);
    }
}
// reciprocals on the device: all 2^23 fp32 mantissas at an even and an odd exponent, then doubles with random low bits at
// exponents -60 .. 60
static void rcp_args(std::vector<double> &a, size_t n) {
    seed(11);
    a.clear();
    for (int e = 0; e <= 1; e++)
        for (uint32_t m = 0; m < (1u << 23); m++) a.push_back(ldexp(1.0 + (double)m * 0x1p-23, e));
    for (size_t i = 0; i < n; i++) a.push_back(from_bits(((uint64_t)(1023 - 60 + (int)(u64() % 121)) << 52) | (u64() >> 12)));
}

// ---- the checks ----------------------------------------------------------------------------------------------------------
struct ExpStat { Worst ulp, rel; long bad = 0; };
static ExpStat check_exp(const std::vector<double> &t, const std::vector<double> &res, int per, int T) {
    std::vector<ExpStat> st(T);
    const ld c = LN2L / (ld)per;
    parallel(t.size(), [&](size_t lo, size_t hi, int s) {
        for (size_t i = lo; i < hi; i++) {
            const ld ref = expl((ld)t[i] * c);
            const ld err = fabsl((ld)res[i] - ref);
            if (!(res[i] > 0.0) || !(res[i] < INFINITY)) st[s].bad++;
            st[s].ulp.take((double)(err / ulp_of(ref)), t[i]);
            st[s].rel.take((double)(err / ref), t[i]);
        }
    }, T);
    ExpStat r;
    for (auto &x : st) { r.ulp.merge(x.ulp); r.rel.merge(x.rel); r.bad += x.bad; }
    return r;
}
struct LogStat { Worst excess, far_ulp, all_ulp, near1; long bad = 0; };
static LogStat check_log(const std::vector<double> &x, const std::vector<double> &res, int T) {
    std::vector<LogStat> st(T);
    parallel(x.size(), [&](size_t lo, size_t hi, int s) {
        for (size_t i = lo; i < hi; i++) {
            const ld ref = logl((ld)x[i]);
            const ld err = fabsl((ld)res[i] - ref), u = ulp_of(ref);
            if (!(res[i] == res[i])) st[s].bad++;
            st[s].excess.take((double)(err - 0.5L * u), x[i]);              // what the absolute term has to carry
            if (fabsl(ref) >= 0.5L) st[s].far_ulp.take((double)(err / u), x[i]);
            if (u > 0.0L) st[s].all_ulp.take((double)(err / u), x[i]);
            if (x[i] >= 1.0 - 1.0 / 128.0 && x[i] < 1.0 + 1.0 / 64.0) st[s].near1.take((double)err, x[i]);
        }
    }, T);
    LogStat r;
    for (auto &q : st) { r.excess.merge(q.excess); r.far_ulp.merge(q.far_ulp); r.all_ulp.merge(q.all_ulp); r.near1.merge(q.near1); r.bad += q.bad; }
    return r;
}
// how log_tab treats what it hands to the library: the sign and kind must be log's; a denormal's value within an ulp
static long check_log_special(const std::vector<double> &res) {
    long bad = 0;
    for (size_t i = 0; i < sizeof(LOG_SPECIAL) / 8; i++) {
        const double x = LOG_SPECIAL[i], r = res[i];
        if (x == 0.0) bad += !(r == -INFINITY);
        else if (x < 0.0 || x != x) bad += !(r != r);
        else if (x == INFINITY) bad += !(r == INFINITY);
        else { const ld ref = logl((ld)x); bad += !(fabsl((ld)r - ref) <= ulp_of(ref)); }
    }
    return bad;
}
struct RcpStat { Worst ulp, rel; };
// kind 0: 1/d, 1: 1/sqrt(d)
static void rcp_err(double d, double y, int kind, RcpStat &s) {
    const ld ref = kind ? 1.0L / sqrtl((ld)d) : 1.0L / (ld)d;
    const ld err = fabsl((ld)y - ref);
    s.ulp.take((double)(err / ulp_of(ref)), d);
    s.rel.take((double)(err / ref), d);
}
static RcpStat check_rcp(const std::vector<double> &d, const std::vector<double> &res, int kind, int T) {
    std::vector<RcpStat> st(T);
    parallel(d.size(), [&](size_t lo, size_t hi, int s) { for (size_t i = lo; i < hi; i++) rcp_err(d[i], res[i], kind, st[s]); }, T);
    RcpStat r;
    for (auto &q : st) { r.ulp.merge(q.ulp); r.rel.merge(q.rel); }
    return r;
}
static long bits_differ(const std::vector<double> &a, const std::vector<double> &b) {
    long n = 0;
    for (size_t i = 0; i < a.size(); i++) n += (to_bits(a[i]) != to_bits(b[i])) && !(a[i] != a[i] && b[i] != b[i]);
    return n;
}

// the five reciprocal results of one argument, as the cut functions give them
static void recips(double d, double out[5]) {
    out[0] = rcp64(d); out[1] = rsqrt64(d);
    rcp_rsqrt(d, out[2], out[3]);
    out[4] = fast_rcp(d);
}
static const char *RCP_NAME[5] = {"rcp64", "rsqrt64", "rr_inv", "rr_rsq", "fast_rcp"};
static const int RCP_KIND[5] = {0, 1, 0, 1, 0};

static void host_eval(const Tables &T, const std::vector<double> &a, std::vector<double> &r, int which, int NT) {
    r.resize(a.size());
    parallel(a.size(), [&](size_t lo, size_t hi, int) {
        for (size_t i = lo; i < hi; i++)
            r[i] = which == 0 ? exp_tab64(a[i], T.et) : which == 1 ? exp_tab256_p3(a[i], T.et256) : log_tab(a[i], T.lt);
    }, NT);
}

static void report_exp(const char *name, const ExpStat &s, size_t n) {
    std::string k(name);
    say((k + "_n").c_str(), (long)n); say((k + "_ulp").c_str(), s.ulp); say((k + "_rel").c_str(), s.rel); say((k + "_bad").c_str(), s.bad);
}
static void report_log(const LogStat &s, size_t n) {
    say("log_n", (long)n); say("log_excess", s.excess); say("log_far_ulp", s.far_ulp); say("log_all_ulp", s.all_ulp);
    say("log_near1_abs", s.near1); say("log_bad", s.bad);
}

// ---- Philox ---------------------------------------------------------------------------------------------------------------
static void philox_report() {
    const unsigned kat[3][6] = {{0, 0, 0, 0, 0, 0},
                                {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                                {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
    for (int i = 0; i < 3; i++) {
        Philox g;
        g.c0 = kat[i][0]; g.c1 = kat[i][1]; g.c2 = kat[i][2]; g.c3 = kat[i][3]; g.k0 = kat[i][4]; g.k1 = kat[i][5]; g.have = 0;
        philox_block(g);
        printf("philox_kat%d %08x %08x %08x %08x have %d c0 %08x\n", i, g.out[0], g.out[1], g.out[2], g.out[3], g.have, g.c0);
    }
    // five uniforms of three streams, as integers U 2^53: the test rebuilds them from its own Philox
    const unsigned long long seeds[3] = {0ull, 1234ull, 0xfedcba9876543210ull}, pix[3] = {0ull, 77ull, (1ull << 63) | 0x123456789ull};
    for (int i = 0; i < 3; i++) {
        Philox g = philox_init(seeds[i], pix[i], (unsigned)(3 * i));
        printf("philox_init%d %08x %08x %08x %08x %08x %08x have %d\n", i, g.c0, g.c1, g.c2, g.c3, g.k0, g.k1, g.have);
        printf("philox_double%d", i);
        for (int k = 0; k < 5; k++) {
            const double u = philox_double(g);
            printf(" %" PRIu64, (uint64_t)(u * 9007199254740992.0));
            if (!(u >= 0.0 && u < 1.0) || u * 9007199254740992.0 != floor(u * 9007199254740992.0)) printf(" OUT-OF-RANGE");
        }
        printf("\n");
    }
    Philox g;
    memset(&g, 0, sizeof g);
    g.out[0] = g.out[1] = g.out[2] = g.out[3] = 0xffffffffu; g.have = 4;
    const double top = philox_double(g), top2 = philox_double(g);
    printf("philox_top %d %d have %d\n", (int)(top == 1.0 - 0x1p-53), (int)(top2 == 1.0 - 0x1p-53), g.have);
    g.out[0] = g.out[1] = g.out[2] = g.out[3] = 0u; g.have = 4;
    printf("philox_bottom %d\n", (int)(philox_double(g) == 0.0));
    g.out[0] = 0x11112222u; g.out[1] = 0x33334444u; g.out[2] = 0x55556666u; g.out[3] = 0x77778888u;
    printf("philox_word");
    for (int w = 0; w < 8; w++) printf(" %04x", philox_word(g, w));
    printf("\n");
}

// ---- modes ----------------------------------------------------------------------------------------------------------------
static int mode_cpu(size_t n) {
    const int NT = n_threads();
    Tables T;
    host_tables(T);
    check_tables(T);
    std::vector<double> a, r;
    exp_args(a, n, 64); host_eval(T, a, r, 0, NT); report_exp("exp64", check_exp(a, r, 64, NT), a.size());
    exp_args(a, n, 256); host_eval(T, a, r, 1, NT); report_exp("exp256", check_exp(a, r, 256, NT), a.size());
    // far below the range: exactly 0 (|t| < 2^31 here: the conversion to int beyond that is the device's to define)
    say("exp_flush_bad", (long)((exp_tab64(-2147483000.0, T.et) != 0.0) + (exp_tab256_p3(-2147483000.0, T.et256) != 0.0) +
                                (exp_tab64(-1e6, T.et) != 0.0) + (exp_tab256_p3(-1e6, T.et256) != 0.0)));
    log_args(a, n); host_eval(T, a, r, 2, NT); report_log(check_log(a, r, NT), a.size());
    {
        std::vector<double> sp(LOG_SPECIAL, LOG_SPECIAL + sizeof(LOG_SPECIAL) / 8), sr;
        host_eval(T, sp, sr, 2, 1);
        long bad = check_log_special(sr);
        for (size_t i = 0; i < sp.size(); i++) {             // and on the host: bit for bit what log returns
            const double l = log(sp[i]);
            bad += !((l != l && sr[i] != sr[i]) || to_bits(l) == to_bits(sr[i]));
        }
        say("log_special_bad", bad);
    }
    // reciprocals: every fp32 mantissa at exponents across 2^-60 .. 2^60 (odd and even), the seed moved by -1, 0, +1 fp32 ulp;
    // then doubles with random low bits
    const int E[] = {-60, -1, 0, 59};
    const size_t M = (size_t)1 << 23, nexp = sizeof(E) / sizeof(E[0]);
    const size_t sweep = n >= 1000000 ? M : (n < 4096 ? 4096 : n);      // (a short run for the mutated copies: a stride through the mantissas)
    std::vector<double> rnd;
    seed(11);
    for (size_t i = 0; i < n; i++) rnd.push_back(from_bits(((uint64_t)(1023 - 60 + (int)(u64() % 121)) << 52) | (u64() >> 12)));
    RcpStat all[5];
    for (int sh = -1; sh <= 1; sh++) {
        g_shift = sh;
        std::vector<RcpStat> st((size_t)NT * 5);
        parallel(sweep * nexp + rnd.size(), [&](size_t lo, size_t hi, int s) {
            double out[5];
            for (size_t i = lo; i < hi; i++) {
                const double d = i < sweep * nexp ? ldexp(1.0 + (double)((i % sweep) * (M / sweep)) * 0x1p-23, E[i / sweep]) : rnd[i - sweep * nexp];
                recips(d, out);
                for (int k = 0; k < 5; k++) rcp_err(d, out[k], RCP_KIND[k], st[(size_t)s * 5 + k]);
            }
        }, NT);
        for (int k = 0; k < 5; k++) {
            RcpStat m;
            for (int s = 0; s < NT; s++) { m.ulp.merge(st[(size_t)s * 5 + k].ulp); m.rel.merge(st[(size_t)s * 5 + k].rel); }
            printf("%s_shift%+d_ulp %.6e %a\n", RCP_NAME[k], sh, m.ulp.v, m.ulp.at);
            printf("%s_shift%+d_rel %.6e %a\n", RCP_NAME[k], sh, m.rel.v, m.rel.at);
            all[k].ulp.merge(m.ulp); all[k].rel.merge(m.rel);
        }
    }
    g_shift = 0;
    for (int k = 0; k < 5; k++) {
        say((std::string(RCP_NAME[k]) + "_ulp").c_str(), all[k].ulp);
        say((std::string(RCP_NAME[k]) + "_rel").c_str(), all[k].rel);
    }
    say("rcp_n", (long)(3 * (sweep * nexp + rnd.size())));
    philox_report();
    return 0;
}

static int mode_gen(const std::string &dir, size_t n) {
    std::vector<double> a;
    bool ok = true;
    exp_args(a, n, 64);
    a.push_back(-1e12); a.push_back(-1e300);               // the last two: far below the range (the conversion to int saturates)
    ok &= write_file(dir + "/exp64.arg", a);
    exp_args(a, n, 256);
    a.push_back(-1e12); a.push_back(-1e300);
    ok &= write_file(dir + "/exp256.arg", a);
    std::vector<double> l;
    log_args(l, n);
    a.assign(LOG_SPECIAL, LOG_SPECIAL + sizeof(LOG_SPECIAL) / 8);      // the special values first
    a.insert(a.end(), l.begin(), l.end());
    ok &= write_file(dir + "/log.arg", a);
    rcp_args(a, n);
    ok &= write_file(dir + "/rcp.arg", a);
    return ok ? 0 : 1;
}

static int mode_check(const std::string &dir) {
    const int NT = n_threads();
    Tables T, H;
    host_tables(H);
    std::vector<double> tab, a, r, h;
    if (!read_file(dir + "/tables.res", tab) || tab.size() != 64 + 256 + 128) { fprintf(stderr, "no tables.res\n"); return 1; }
    memcpy(T.et, tab.data(), sizeof T.et); memcpy(T.et256, tab.data() + 64, sizeof T.et256); memcpy(T.lt, tab.data() + 320, sizeof T.lt);
    check_tables(T);
    say("tab_bits_differ", (long)(bits_differ(std::vector<double>(T.et, T.et + 64), std::vector<double>(H.et, H.et + 64)) +
                                  bits_differ(std::vector<double>(T.et256, T.et256 + 256), std::vector<double>(H.et256, H.et256 + 256))));
    say("tab_lt_bits_differ", bits_differ(std::vector<double>(T.lt, T.lt + 128), std::vector<double>(H.lt, H.lt + 128)));
    for (int per = 64; per <= 256; per *= 4) {
        const std::string nm = per == 64 ? "exp64" : "exp256";
        if (!read_file(dir + "/" + nm + ".arg", a) || !read_file(dir + "/" + nm + ".res", r) || a.size() != r.size() || a.size() < 2) {
            fprintf(stderr, "no %s files\n", nm.c_str()); return 1;
        }
        long flush_bad = 0;
        for (int k = 0; k < 2; k++) { flush_bad += !(r.back() == 0.0) || std::signbit(r.back()); a.pop_back(); r.pop_back(); }
        report_exp(nm.c_str(), check_exp(a, r, per, NT), a.size());
        say((nm + "_flush_bad").c_str(), flush_bad);
        host_eval(H, a, h, per == 64 ? 0 : 1, NT);
        say((nm + "_bits_differ").c_str(), bits_differ(r, h));
    }
    if (!read_file(dir + "/log.arg", a) || !read_file(dir + "/log.res", r) || a.size() != r.size()) { fprintf(stderr, "no log files\n"); return 1; }
    const size_t ns = sizeof(LOG_SPECIAL) / 8;
    say("log_special_bad", check_log_special(r));
    a.erase(a.begin(), a.begin() + ns); r.erase(r.begin(), r.begin() + ns);
    report_log(check_log(a, r, NT), a.size());
    host_eval(H, a, h, 2, NT);
    say("log_bits_differ", bits_differ(r, h));
    if (!read_file(dir + "/rcp.arg", a)) { fprintf(stderr, "no rcp.arg\n"); return 1; }
    for (int k = 0; k < 5; k++) {
        if (!read_file(dir + "/" + RCP_NAME[k] + ".res", r) || r.size() != a.size()) { fprintf(stderr, "no %s.res\n", RCP_NAME[k]); return 1; }
        const RcpStat s = check_rcp(a, r, RCP_KIND[k], NT);
        say((std::string(RCP_NAME[k]) + "_ulp").c_str(), s.ulp);
        say((std::string(RCP_NAME[k]) + "_rel").c_str(), s.rel);
        h.resize(a.size());
        parallel(a.size(), [&](size_t lo, size_t hi, int) { double o[5]; for (size_t i = lo; i < hi; i++) { recips(a[i], o); h[i] = o[k]; } }, NT);
        say((std::string(RCP_NAME[k]) + "_bits_differ").c_str(), bits_differ(r, h));
    }
    say("rcp_n", (long)a.size());
    return 0;
}

int main(int argc, char **argv) {
    printf("ldbl_mant_dig %d\n", (int)LDBL_MANT_DIG);
    if (LDBL_MANT_DIG < 64) { fprintf(stderr, "long double has a %d-bit mantissa: no reference here\n", (int)LDBL_MANT_DIG); return 3; }
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "cpu" && argc > 2) return mode_cpu((size_t)atol(argv[2]));
    if (mode == "gen" && argc > 3) return mode_gen(argv[2], (size_t)atol(argv[3]));
    if (mode == "check" && argc > 2) return mode_check(argv[2]);
    fprintf(stderr, "usage: primitives_exact cpu N | gen DIR N | check DIR\n");
    return 2;
}
