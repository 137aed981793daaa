"""The math primitives under every kernel, pinned to exact references: exp_tab64, exp_tab256_p3, log_tab, rcp64, rsqrt64,
rcp_rsqrt (k_render.h), fast_rcp and the Philox routines (k_split.h).

Nine kernel headers call them at 64 sites, and the contract tests (test_drop_contract.py, test_conditional_contract.py) build
their tolerances on the accuracy these functions claim; the rest of the suite sees them only through sums at 1e-9 .. 1e-12.
Here each function is held, argument by argument, to a bound derived below -- never to a measurement rounded up -- against
arithmetic with a 64-bit mantissa (x87 long double: expl, logl, division, sqrtl; LDBL_MANT_DIG >= 64 is asserted).

  CPU     the functions cut from the shipped headers between their "[prim-checked: ...]" marks and compiled as plain C++
          without contraction (tests/host/primitives_exact.cpp); the fp32 instructions v_rcp_f32 / v_rsq_f32 stood in for by
          the correctly rounded fp32 value moved by -1, 0 and +1 fp32 ulp.
  device  the same headers compiled with the library's flags into tools/bin/prim_probe (tests/device/prim_probe.hip, the
          `probe` target of csrc/Makefile), run ONCE as a child process on files of arguments; its result files go through
          the same references and the same bounds, its tables through the entry bounds the derivations assume.
  Philox  the three published Philox4x32-10 known answers through philox_block; philox_double's order, formula and range;
          philox_word's eight half-words; and the shipped library's own stream through cel_debug_binomial(n = 1), which
          shows on which side of j/256 the first uniform of every stream falls.

Notation: u = 2^-53; a rounding to nearest is <= u relative and <= half an ulp; an "ulp" is that of the fp64 binade holding the
exact value; a relative error e is at most e / u ulp (an ulp is more than u of its value) -- the 2^-53-to-ulp conversion.  The
reference's own error: expl / logl / the long-double quotient are within 2^-63 relative, 2^-10 ulp of fp64: REF below.

exp_tab64(t) = ldexp(et[n & 63] * p(f), n >> 6), n = rint(t), f = t - n (exact), |f| <= 1/2, r = f ln2/64, |r| <= ln2/128.
  table entry     T ulp of 2^(j/64): <= 2 T u relative (T = 1/2 for a correctly rounded entry, 1 for the device's exp2)
  coefficients    each correctly rounded, u relative: together <= u (e^|r| - 1) = 0.0055 u
  the four inner fma   a rounding of a value <= 1.09e-2, then multiplied by |f| <= 1/2, the earlier ones by more powers:
                       <= 0.0055 u
  the last fma    p in [0.9946, 1.0055]: <= u relative
  truncation      degree 5: r^6/720 e^|r| / e^-|r| <= 3.56e-17 = 0.321 u
  the product     et * p: <= u;   ldexp: exact for a normal result
  sum             (2 T + 2.333) u  ->  EXP64_ULP(T) = 2 T + 2.34 ulp: 3.34 on a correctly rounded table, 4.34 within 1 ulp.
exp_tab256_p3: the same with a cubic, |r| <= ln2/512 = 1.3538e-3:
  truncation      r^4/24 e^|r| = 1.3996e-13 * 1.00136 = 1.4015e-13 relative
  table entry     e64 (2 T u) times a correctly rounded constant (u), the product rounded (u): (2 T + 2) u
  polynomial      u (1 + 0.003), product u
  sum             EXP256_REL(T) = 1.4015e-13 + (2 T + 4.01) u: 1.4071e-13 for T = 1/2, 1.4083e-13 for T = 1.
  Both: exactly 0 far below the range (ldexp flushes; on the device the conversion of n to int saturates).
log_tab(x) = fma(e, HI, lc[j] + fma(e, LO, p)), x = 2^e m, r = fma(m, ic[j], -1), |r| < 2^-7, p = log1p's series to r^7.
  r               one rounding of a value below 2^-7: <= 2^-61 = 4.4e-19 (log1p' <= 1.008)
  series          truncation r^8/8/(1 - |r|) <= 1.76e-18; the last fma's rounding u times |r| = 8.7e-19, the product p * r
                  8.7e-19, the earlier ones (times r^2 and beyond) and the coefficients' < 1e-20        together 3.95e-18
  fma(e, LO, p)   a value below 2^-7: <= 2^-61 = 4.4e-19; LO's own rounding 2^-86 |e| < 2e-23
  lc[j]           the entry, < 1: <= 2^-54 (half an ulp of -log(ic[j]), which the identity is exact for)
  lc[j] + ...     a sum below 1: <= 2^-54
  the last fma    e * HI is exact (HI has 32 bits): half an ulp of the RESULT
  sum             |err| <= 0.5 ulp(result) + LOG_ABS, LOG_ABS = 2 * 2^-54 + 4.4e-19 + 4.4e-19 + 3.95e-18 = 1.159e-16.
  So the error is ABSOLUTE near x = 1 (many ulp of a small result: 40 ulp just below 1, where e ln2 cancels against lc[63]),
  and where |log x| >= 0.5 (an ulp >= 2^-53) it is <= 0.5 + 1.05 ulp by this sum; the contract tests quote 1.5 ulp there,
  which is asserted as such (for e = 0 the last fma does not round, for e = -1 and |log x| >= 0.5 the two 2^-54 are 2^-56).
rcp64(d): y0 = rcp_f32((float)d) = (1/d)(1 + e0), |e0| <= 2^-24 (the conversion) + 2^-24 (correct rounding) + 2^-23 (one fp32
  ulp off) = 2^-22.  A step y + y fma(-d, y, 1): the residual is ONE rounding of 1 - d y = -e0 (relative u: 3e-23), the outer
  fma one rounding: e1 <= e0^2 + 1.01 u = 5.70e-14 -- that is fast_rcp: FAST_RCP_REL = 2^-44 + 1.01 * 2^-53.
  Second step: e1^2 + e1 u = 3.3e-27 before the last rounding: RCP_ULP = 0.5 + 3e-11 (+ REF).
rsqrt64(d): z0 = (1/sqrt d)(1 + e0), |e0| <= 2^-25 + 1.5 * 2^-23 = 1.94e-7.  A step z fma(-0.5 d z, z, 1.5) in exact arithmetic
  gives 1 - 1.5 e^2 - 0.5 e^3; -0.5 d is exact, (-0.5 d) z rounds (u relative of 1/2: u/2 absolute in the fma's sum), the fma
  rounds a value next to 1 (<= u), the product rounds (half an ulp of the result).  After the first step e1 <= 5.7e-14; after
  the second 1.5 u + 1.5 e1^2 relative = 1.5 ulp at most, plus the half ulp: RSQRT_ULP = 2.0 (+ 5e-11 + REF).
  rcp_rsqrt is the two together: the same bounds.

MEASURED (the worst case of each run is printed; the bounds above are what is asserted)
  CPU, 10^7 random arguments per function + the edge sets; reciprocals: 2^23 mantissas x 4 exponents x 3 seed shifts + 10^7
    exp_tab64 2.30 ulp | exp_tab256_p3 1.4051e-13 | log_tab 1.110e-16 beyond the half ulp, 0.994 ulp where |log x| >= 0.5,
    6.56e-17 absolute on [1 - 1/128, 1 + 1/64), 3.5e13 ulp of the result at 1 + 2^-51 | rcp64 0.5000 ulp | rsqrt64 1.966 ulp
    | fast_rcp 4.34e-14 (seed one ulp off), 7.96e-15 (correctly rounded seed)
  MI355X, 10^6 random arguments per function + the edge sets; reciprocals: 2^23 mantissas x 2 exponents + 10^6
    table entries within 0.565 ulp (64) and 2.39 u (256); the log table equal to the host's in every bit
    exp_tab64 2.23 ulp | exp_tab256_p3 1.4048e-13 | both exactly +0 at t = -1e12 and -1e300 | log_tab 1.110e-16 beyond the half
    ulp, 0.990 ulp where |log x| >= 0.5, 6.56e-17 absolute near 1, every result equal in bits to the host-cut function's |
    rcp64 0.5000 ulp, equal in bits to the host's with a correctly rounded seed | rsqrt64 1.896 ulp | fast_rcp 1.449e-14:
    v_rcp_f32 delivers about half an fp32 ulp here, and one Newton step cannot give the 4e-15 the comments used to claim
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "desi-mcmc_amd", "csrc")
PROBE = os.path.join(ROOT, "tools", "bin", "prim_probe")
BEGIN, END = "// [prim-checked: begin]", "// [prim-checked: end]"
CUTS = (("device_common.h", "prim_common.inc"), ("k_render.h", "prim_render.inc"), ("k_split.h", "prim_split.inc"))

U = 2.0 ** -53
REF = 2.0 ** -10                                   # the long-double reference's own error, in fp64 ulp
EXP64_ULP = lambda T: 2.0 * T + 2.34 + REF
EXP256_REL = lambda T: 1.4015e-13 + (2.0 * T + 4.01) * U + REF * U
TAB256_RELU = lambda T: 2.0 * T + 2.0 + REF        # an entry of the 256 table, in units of u relative
LOG_ABS = 2 * 2.0 ** -54 + 2 * 2.0 ** -61 + 3.95e-18
LOG_FAR_ULP = 1.5                                  # where |log x| >= 0.5: what the contract tests quote
RCP_ULP = 0.5 + 3e-11 + REF
RSQRT_ULP = 2.0 + 5e-11 + REF
FAST_RCP_REL = 2.0 ** -44 + 1.01 * U

KNOWN_ANSWERS = (      # Philox4x32-10 (Salmon et al. 2011; the Random123 known-answer file): counter, key -> output
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
)


# ---------------------------------------------------------------------------------------------------------------------
# a plain Philox4x32-10 of the test's own (numpy, any number of counters at once)
def philox4x32(counter, key, rounds=10):
    m32 = np.uint64(0xffffffff)
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & m32 for c in counter)
    k0, k1 = (np.uint64(k) for k in key)
    s32 = np.uint64(32)
    for _ in range(rounds):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def uniform53(hi, lo):
    """philox_double's formula as an integer: U 2^53 = (hi >> 5) 2^26 + (lo >> 6)"""
    return ((np.asarray(hi, np.uint64) >> np.uint64(5)) << np.uint64(26)) | (np.asarray(lo, np.uint64) >> np.uint64(6))


def first_uniforms(seed, N):
    """U_i 2^53 for the first uniform of stream i of cel_debug_binomial: key = the seed's halves, counter = (0, 0, i lo, i hi)"""
    i = np.arange(N, dtype=np.uint64)
    w = philox4x32((np.zeros(N, np.uint64), np.zeros(N, np.uint64), i & np.uint64(0xffffffff), i >> np.uint64(32)),
                   (seed & 0xffffffff, seed >> 32))
    return uniform53(w[3], w[2])


def test_the_tests_philox_reproduces_the_known_answers():
    for counter, key, words in KNOWN_ANSWERS:
        assert " ".join("%08x" % int(w) for w in philox4x32(counter, key)) == words


# ---------------------------------------------------------------------------------------------------------------------
# the functions as cut from the headers, on the CPU
def cut_spans():
    out = {}
    for header, inc in CUTS:
        src, spans, at = open(os.path.join(CSRC, header)).read(), [], 0
        while src.find(BEGIN, at) >= 0:
            a = src.index(BEGIN, at)
            at = src.index(END, a)
            spans.append(src[a:at])
        assert spans, header
        out[inc] = "\n".join(spans)
    for name in ("exp_tab64", "exp_tab256_p3", "exp_tab256_fill", "log_tab", "rcp64", "rsqrt64", "rcp_rsqrt"):
        assert "inline double %s(" % name in out["prim_render.inc"] or "inline void %s(" % name in out["prim_render.inc"], name
    for name in ("struct Philox", "void philox_block(", "Philox philox_init(", "double philox_double(", "unsigned philox_word(",
                 "double fast_rcp("):
        assert name in out["prim_split.inc"], name
    assert "void log_tab_fill(" in out["prim_common.inc"]
    return out


def compile_host(where, texts, strict=True):
    for inc, text in texts.items():
        with open(os.path.join(str(where), inc), "w") as f:
            f.write(text)
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(where), "primitives_exact")
    # no contraction: the marked functions spell out every fma they mean
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra"] + (["-Werror"] if strict else []) +
                   ["-Wno-unknown-pragmas", "-pthread", "-I", str(where), os.path.join(ROOT, "tests", "host", "primitives_exact.cpp"),
                    "-o", exe], check=True, capture_output=True, text=True)
    return exe


def parse(stdout):
    st = {}
    for line in stdout.splitlines():
        w = line.split()
        if w:
            st[w[0]] = w[1:]
    return st


def val(st, key):
    return float(st[key][0])


def check_tables(st, T):
    """the entries against exact 2^(j/64), 2^(j/256), 1/c_j and -log(ic[j]), within what the derivations assume for them"""
    assert val(st, "tab_et64_ulp") <= T + REF, st["tab_et64_ulp"]
    assert val(st, "tab_et256_relu") <= TAB256_RELU(T), st["tab_et256_relu"]
    assert val(st, "tab_ic_ulp") <= 0.5 + REF, st["tab_ic_ulp"]
    assert val(st, "tab_lc_ulp") <= 0.5 + REF, st["tab_lc_ulp"]


def check_functions(st, T, n_random):
    """the bounds of the module docstring on one run's worst cases (T: the 64-entry table's error in its ulp)"""
    assert int(st["ldbl_mant_dig"][0]) >= 64, "no 64-bit-mantissa reference on this machine"
    for name in ("exp64", "exp256", "log"):
        assert int(st[name + "_n"][0]) >= n_random and int(st[name + "_bad"][0]) == 0, name
    assert val(st, "exp64_ulp") <= EXP64_ULP(T), st["exp64_ulp"]
    assert val(st, "exp256_rel") <= EXP256_REL(T), st["exp256_rel"]
    assert val(st, "log_excess") <= LOG_ABS, st["log_excess"]
    assert val(st, "log_far_ulp") <= LOG_FAR_ULP, st["log_far_ulp"]
    assert val(st, "log_near1_abs") <= LOG_ABS + 2.0 ** -60, st["log_near1_abs"]      # |log x| < 2^-6 there: half an ulp is at most 2^-60
    assert int(st["log_special_bad"][0]) == 0
    for name in ("rcp64", "rr_inv"):
        assert val(st, name + "_ulp") <= RCP_ULP, (name, st[name + "_ulp"])
    for name in ("rsqrt64", "rr_rsq"):
        assert val(st, name + "_ulp") <= RSQRT_ULP, (name, st[name + "_ulp"])
    assert val(st, "fast_rcp_rel") <= FAST_RCP_REL, st["fast_rcp_rel"]


def check_philox(st):
    for i, (counter, key, words) in enumerate(KNOWN_ANSWERS):
        got = st["philox_kat%d" % i]
        assert " ".join(got[:4]) == words, (i, got)
        assert got[4:] == ["have", "4", "c0", "%08x" % ((counter[0] + 1) & 0xffffffff)], got      # four words, the next block's counter
    seeds, pixels = (0, 1234, 0xfedcba9876543210), (0, 77, (1 << 63) | 0x123456789)
    for i, (seed, pixel) in enumerate(zip(seeds, pixels)):
        g = [int(w, 16) for w in st["philox_init%d" % i][:6]]
        assert g == [0, 3 * i, pixel & 0xffffffff, pixel >> 32, seed & 0xffffffff, seed >> 32] and st["philox_init%d" % i][6:] == ["have", "0"]
        # words (3, 2), then (1, 0), then a new block with c0 + 1
        want = []
        for blk in range(3):
            w = philox4x32((g[0] + blk, g[1], g[2], g[3]), (g[4], g[5]))
            want += [int(uniform53(w[3], w[2])), int(uniform53(w[1], w[0]))]
        assert [int(x) for x in st["philox_double%d" % i]] == want[:5], (i, st["philox_double%d" % i], want)      # (also: no OUT-OF-RANGE word)
    assert st["philox_top"] == ["1", "1", "have", "0"]          # both pairs of an all-ones block: 1 - 2^-53, the largest value, below 1
    assert st["philox_bottom"] == ["1"]
    assert st["philox_word"] == ["2222", "1111", "4444", "3333", "6666", "5555", "8888", "7777"]


def run_host(exe, *args):
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    return run.stdout


N_CPU = 10 ** 7


def test_cut_functions_meet_their_bounds(tmp_path):
    exe = compile_host(tmp_path, cut_spans())
    out = run_host(exe, "cpu", N_CPU)
    print(out)
    st = parse(out)
    check_tables(st, 0.5)
    check_functions(st, 0.5, N_CPU)
    assert int(st["exp_flush_bad"][0]) == 0
    assert int(st["rcp_n"][0]) >= 3 * (4 * 2 ** 23 + N_CPU)
    for shift in ("-1", "+0", "+1"):                      # the bounds hold for every stand-in of the fp32 instruction
        for name, kind, bound in (("rcp64", "ulp", RCP_ULP), ("rr_inv", "ulp", RCP_ULP), ("rsqrt64", "ulp", RSQRT_ULP),
                                  ("rr_rsq", "ulp", RSQRT_ULP), ("fast_rcp", "rel", FAST_RCP_REL)):
            assert val(st, "%s_shift%s_%s" % (name, shift, kind)) <= bound, (name, shift)
    check_philox(st)


def _rcp64_one_step(text):
    a = text.index("inline double rcp64(")
    body = "    y = fma(y, fma(-d, y, 1.0), y);\n    return fma(y, fma(-d, y, 1.0), y);"
    assert text.index(body, a) < text.index("inline double rsqrt64(")
    return text[:a] + text[a:].replace(body, "    return fma(y, fma(-d, y, 1.0), y);", 1)


MUTATIONS = {
    "c5 removed from exp_tab64": ("prim_render.inc", lambda t: t.replace("double p = fma(f, c5, c4);", "double p = c4;", 1)),
    "ni >> 6 written as ni / 64": ("prim_render.inc", lambda t: t.replace("ni >> 6)", "ni / 64)", 1)),
    "LN2_LO dropped": ("prim_render.inc", lambda t: t.replace("fma(e, LN2_LO, p)", "p", 1)),
    "one Newton step removed from rcp64": ("prim_render.inc", _rcp64_one_step),
    "the two Philox multipliers swapped": ("prim_split.inc", lambda t: t.replace("0xD2511F53u", "0xTMP").replace("0xCD9E8D57u", "0xD2511F53u")
                                           .replace("0xTMP", "0xCD9E8D57u")),
    "philox_double taking words (1, 0) first": ("prim_split.inc", lambda t: t.replace("first = (g.have == 4)", "first = (g.have != 4)", 1)),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_a_mutated_copy_fails(tmp_path, name):
    """the checks above notice each of these changes to the cut text (a short run: 20 000 random arguments and a stride through
    the mantissas are enough for all six)"""
    texts = cut_spans()
    inc, change = MUTATIONS[name]
    mutated = change(texts[inc])
    assert mutated != texts[inc], "the mutation no longer applies: " + name
    texts[inc] = mutated
    st = parse(run_host(compile_host(tmp_path, texts, strict=False), "cpu", 20000))
    with pytest.raises(AssertionError):
        check_functions(st, 0.5, 20000)
        check_philox(st)


# ---------------------------------------------------------------------------------------------------------------------
# the same functions on the device
N_DEVICE = 10 ** 6


def probe_binary():
    """tools/bin/prim_probe, built by the library's Makefile (`make probe`, part of `all`) when missing or older than a header"""
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith(".h"))
    newest = max(newest, os.path.getmtime(os.path.join(ROOT, "tests", "device", "prim_probe.hip")))
    if not os.path.exists(PROBE) or os.path.getmtime(PROBE) < newest:
        subprocess.run(["make", "-C", CSRC, "-s", "probe"], check=True, capture_output=True, text=True, timeout=600)
    return PROBE


@pytest.mark.gpu
def test_device_functions_meet_the_same_bounds(tmp_path):
    probe = probe_binary()
    exe = compile_host(tmp_path, cut_spans())
    work = tmp_path / "run"
    work.mkdir()
    run_host(exe, "gen", work, N_DEVICE)
    # once, in a process of its own, under a time limit; after a failure nothing else is started
    run = subprocess.run([probe, str(work)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, "prim_probe failed (%d): %s" % (run.returncode, run.stderr[-2000:])
    out = run_host(exe, "check", work)
    print(run.stdout + out)
    st = parse(out)
    # the device's 64-entry table is exp2's: within 1 ulp is what the derivations allow it; the log table is the host's
    check_tables(st, 1.0)
    assert int(st["tab_lt_bits_differ"][0]) == 0
    check_functions(st, 1.0, N_DEVICE)
    assert int(st["rcp_n"][0]) == 2 * 2 ** 23 + N_DEVICE
    # t = -1e12 and t = -1e300: exactly +0, not NaN
    assert int(st["exp64_flush_bad"][0]) == 0 and int(st["exp256_flush_bad"][0]) == 0
    # informative: results that differ in bits from the host-cut functions (contraction, exp2 and the fp32 instructions may differ)
    print("bits differ from the host-cut functions:", {k[:-12]: int(v[0]) for k, v in st.items() if k.endswith("_bits_differ")})


# ---------------------------------------------------------------------------------------------------------------------
# the shipped library's Philox through its own entry point
# cel_debug_binomial(ctx, 1, p, seed, N, out) draws Binomial(1, p) from stream i = philox_init(seed, i, 0): with p = j/256,
# r = min(p, 1 - p) and 1 - r are exact, and the inversion returns 0 when U <= 1 - r, again 0 when U <= qn = exp(log(1 - r)) -- within
# a few 2^-53 of 1 - r -- and 1 otherwise.  So out[i] = [U_i > 1 - p] for j <= 128 and, flipped, [U_i <= p] above, for every U_i
# further than that from j/256 (and from 1, where the tail restart would draw again).
SEEDS = (0, 1234, 2 ** 32 + 5, 2 ** 64 - 1)
N_STREAMS = 65536


def test_no_first_uniform_lies_at_a_boundary():
    for seed in SEEDS:
        u = first_uniforms(seed, N_STREAMS).astype(np.int64)
        cell = 2 ** 45                                                  # j/256 in units of 2^-53
        off = (u + cell // 2) % cell - cell // 2                        # signed distance to the nearest multiple of 1/256, 1 included
        assert np.abs(off).min() > 2 ** 13, seed                        # 2^-40


@pytest.mark.gpu
def test_library_streams_fall_where_philox_says():
    import desi_mcmc_amd as cel
    from desi_mcmc_amd import _lib
    ctx = cel.Context(0)
    out = np.zeros(N_STREAMS, np.int64)
    for seed in SEEDS:
        u = first_uniforms(seed, N_STREAMS).astype(np.int64)
        for j in range(1, 256):
            out[:] = -1
            _lib.check(_lib.lib().cel_debug_binomial(ctx._h, 1, j / 256.0, seed, N_STREAMS, out.ctypes.data_as(_lib.c_int64_p)))
            want = (u > (256 - j) * 2 ** 45) if j <= 128 else (u <= j * 2 ** 45)
            wrong = np.flatnonzero(out != want)
            assert wrong.size == 0, (seed, j, wrong[:5], out[wrong[:5]], u[wrong[:5]])
