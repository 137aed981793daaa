"""A seeded random walk over the calls that share one long-lived ImageSet + SourceSet (the "live" pair), for tests/test_state_walk.py.

Three parts.

ops(seed, steps, flavour)   a pure-Python generator of operation sequences: it imports neither the library nor numpy, keeps an
                            ABSTRACT state (which pixels are loaded, the option values, whether a resident split exists) and
                            says for every call whether the documentation has it refused (`expect`).
the host mirror `cur`       of the catalogue: host edits are applied to it first, and after every device sampler it is read
                            back with SourceSet.get(), so it stays bit exact.
the replay reference        for every operation that returns numbers: FRESH ImageSet / SourceSet objects on the same context,
                            fed the shortest recipe that legitimately reaches the same inputs, asked the same question, and
                            dropped.  The reference is the same library without memory, so every comparison is bit for bit
                            (stamp masses besides: also against an object that never had a split, to the short cut's bound).

The replay rule, now that the walk also changes what every cached product depends on (the row window, the owned rows, the
context's options):
  * the fresh pair is given today's window and owned rows FIRST, before any call (Walker.fresh);
  * a resident split is replayed with its own catalogue and seed and with the options OF ITS TIME (Walker.time_options: the
    earlier snapshot extended by both thresholds and the kernel variant, and -- the header has them "agree to rounding between
    settings", so the totals behind a split are a product of their time too -- by CEL_OPT_TILE_PARTS and CEL_OPT_STAR_TILES).
    Its draws are a product of their time.  A split made under another window is never replayed: the generator's model, like
    the library, says there is none;
  * every deterministic reader -- the render in either form, model_images, stamp_mass / _begin / _end, estep, grad, pll,
    source_boxes, and the split's totals via split_rates() -- is compared with a fresh computation under TODAY's options: a live
    pair that answers from a product of another threshold, variant or window shows up as a bit difference.  Right after a split,
    split_rates() equals that of a fresh pair that made EVERYTHING at the options in force at the split;
  * the replay never sees the history of CEL_OPT_TILE_ORDER and CEL_OPT_SLICE_FUSE (nor, for the deterministic readers, of
    CEL_OPT_TILE_PARTS and CEL_OPT_STAR_TILES): it is built under today's values, and no equality across values is asserted.
A model image of one threshold under a split at another is "cold" by the documented rule, like a new sky level: the generator
calls that split split_cold, and its replay renders nothing first (the two forms of the totals agree to 1e-10, not bit for bit:
CEL_OPT_SPLIT_REUSE).

The walker runs on a Context of its own: its option flips never reach the session's shared context.
"""
import random

# ---- the generator ---------------------------------------------------------------------------------------------------------------
SET_ROWS = ("set_rows_1", "set_rows_3", "set_rows_20", "set_rows_70")
SAMPLERS = ("flux", "slice_locations", "slice_sample0_comp", "slice_sample0_dirs", "slice_sample1", "type_move")
EXACT = ("exact_slice0", "exact_slice1", "exact_type_move")
OPTIONS = ("opt_incremental", "opt_split_reuse", "opt_honour_mask", "opt_split_full_box")
#: the operations of the "gibbs" and "edits" walks (their window_to comes with the windowed refusal alone) ...
BASE_OPERATIONS = SET_ROWS + ("set", "render", "render_noll", "split_traced", "split_cold", "mass", "mass_begin", "mass_end") + SAMPLERS \
    + EXACT + ("pll", "pll_isolated", "estep", "grad", "set_epsilon", "set_nelec") + OPTIONS
#: ... and the inputs every cached product depends on, walked by "strips" and "options": the row window, the owned rows, the
#: context options that change results (thresholds, kernel variant) and those that must not (tile order, tile parts, slice fuse),
#: the observed pixels' address handed out
INPUTS = ("window_to", "noise_rows", "opt_tail", "opt_kernel", "opt_tile_order", "opt_tile_parts", "opt_slice_fuse", "hand_out")
#: every operation of the walk (what the coverage counts)
OPERATIONS = BASE_OPERATIONS + INPUTS
#: the walk on the stars_only scene: what keeps a catalogue without galaxies one, and CEL_OPT_STAR_TILES
STAR_OPERATIONS = SET_ROWS + ("set", "render", "render_noll", "split_traced", "split_cold", "mass", "mass_begin", "mass_end", "flux", "slice_locations",
                              "pll", "estep", "grad", "set_epsilon", "opt_incremental", "opt_split_reuse", "noise_rows", "opt_tail", "opt_tile_order",
                              "opt_tile_parts", "opt_star_tiles", "hand_out")
WINDOWS = ((0, 192), (32, 256), (64, 256), (0, 256))       # (y0, full_H) of cel_images_set_window: none, a strip inside, the last strip, the first
NOISE_ROWS = ((0, 192), (0, 64), (64, 128), (64, 192))     # owned rows: all, and what 64-row render tiles allow a log-likelihood
#: CEL_OPT_TAIL_LOG's presets, CEL_OPT_TAIL_LOG_SOURCE = 8 alone and CEL_OPT_TAIL_LOG = 8 (both): a component is dropped below
#: e^-8 = 3e-4 of a sky pixel, so a product of the coarse threshold misses the others by orders of magnitude above rounding
TAILS = ("default", "strict", "fast", "source8", "all8")
#: what may run while the context is on the direct kernels: the deterministic readers and the inputs.  A split or a sampler
#: under CEL_OPT_KERNEL = 0 is other tests' subject; the generator returns to the recurrence first
DIRECT_OK = SET_ROWS + ("set", "render", "render_noll", "mass", "mass_begin", "mass_end", "estep", "grad", "set_epsilon", "set_nelec") + OPTIONS + INPUTS \
    + ("opt_star_tiles",)


def tail_of(now, name):
    """(field render's threshold, per-source threshold) after opt_tail `name` from `now`"""
    return {"default": (24.0, 32.0), "strict": (32.0, 32.0), "fast": (20.0, 20.0), "source8": (now[0], 8.0), "all8": (8.0, 8.0)}[name]


#: what "strips" and "options" owe: the inputs, and the products and readers that depend on them (the masked sets, the exact
#: conditional and the rest of BASE_OPERATIONS come as the weights have them: "gibbs" and "edits" owe those)
INPUT_OPERATIONS = INPUTS + ("set_rows_1", "set_rows_3", "render", "render_noll", "split_traced", "split_cold", "mass", "mass_begin", "mass_end") \
    + SAMPLERS + ("pll", "estep", "grad", "set_epsilon")


def required(flavour):
    return {"gibbs": BASE_OPERATIONS, "edits": BASE_OPERATIONS, "stars": STAR_OPERATIONS}.get(flavour, INPUT_OPERATIONS)


#: the documented refusals: a masked set without CEL_OPT_HONOUR_MASK (split, flux); slice_*, the type move and the isolated
#: patch_loglik on any masked set; the exact conditional on a windowed set; no resident split; _end behind a rebuilt catalogue
REFUSALS = ("masked_unhonoured", "masked_sampler", "window", "no_split", "end_rebuilt")
PATTERNS = ("pattern_dirty", "pattern_ready", "pattern_end_rebuilt", "pattern_eps")
#: ("strips", "options") a product, then the input it depends on changed, then its reader
INPUT_PATTERNS = ("pattern_tail_split", "pattern_tail_mass", "pattern_window_split", "pattern_rows_dirty", "pattern_kernel_dirty")
PROBES = ("probe_no_split", "probe_masked_unhonoured", "probe_masked_sampler", "probe_window")

_W_COMMON = {"set": 2, "render_noll": 2, "mass_begin": 3, "pll": 3, "pll_isolated": 2, "estep": 2, "grad": 2, "set_epsilon": 3, "set_nelec": 2,
             "opt_incremental": 1, "opt_split_reuse": 1, "opt_honour_mask": 2, "opt_split_full_box": 1,
             "pattern_dirty": 2, "pattern_ready": 2, "pattern_end_rebuilt": 2, "pattern_eps": 2}
FLAVOURS = {
    # sampler-heavy: the sweep of a Gibbs chain in any order
    "gibbs": dict(_W_COMMON, **{"set_rows_1": 3, "set_rows_3": 2, "set_rows_20": 1, "set_rows_70": 1, "render": 5, "split_traced": 5, "split_cold": 4,
                                "mass": 6, "flux": 8, "slice_locations": 7, "slice_sample0_comp": 4, "slice_sample0_dirs": 4, "slice_sample1": 6,
                                "type_move": 7, "exact_slice0": 3, "exact_slice1": 3, "exact_type_move": 3}),
    # render / set_rows-heavy: the single-source moves of a host-side chain between the device's steps
    "edits": dict(_W_COMMON, **{"set_rows_1": 12, "set_rows_3": 8, "set_rows_20": 5, "set_rows_70": 3, "render": 18, "render_noll": 5, "split_traced": 3,
                                "split_cold": 3, "mass": 4, "flux": 3, "slice_locations": 2, "slice_sample0_comp": 1, "slice_sample0_dirs": 1,
                                "slice_sample1": 2, "type_move": 3, "exact_slice0": 1, "exact_slice1": 1, "exact_type_move": 1}),
}
_W_INPUTS = {"window_to": 2, "noise_rows": 2, "opt_tail": 2, "opt_kernel": 1, "opt_tile_order": 1, "opt_tile_parts": 2, "opt_slice_fuse": 1, "hand_out": 1}
# the row-strip deal's inputs under every sampler and the render
FLAVOURS["strips"] = dict(FLAVOURS["gibbs"], **dict(_W_INPUTS, window_to=14, noise_rows=12, render=12, set_rows_1=5, hand_out=3))
# the context's options between a product and its reader
FLAVOURS["options"] = dict(FLAVOURS["edits"], **dict(_W_INPUTS, opt_tail=14, opt_kernel=5, opt_tile_order=5, opt_tile_parts=8, opt_slice_fuse=4,
                                                    split_traced=9, split_cold=7, mass=12, flux=5, slice_locations=4))
FLAVOURS["stars"] = {k: {"render": 10, "set_rows_1": 6, "opt_star_tiles": 8, "split_traced": 4, "mass": 4, "flux": 4, "opt_tile_parts": 4}.get(k, 2)
                     for k in STAR_OPERATIONS}
NEED = 3            # every operation at least so often


class _Abstract(object):
    """what the generator knows about the live pair without running anything"""

    def __init__(self):
        self.nelec = 0                  # 0 plain, 1 one pixel above 65 535, 2 a few NaNs (a MASKED set)
        self.inc, self.reuse, self.honour, self.full = 1, 2, 0, 0
        self.split = None               # dict(full=, dirty=, sums=, tail=) of the resident split, None without one
        self.window, self.noise = WINDOWS[0], NOISE_ROWS[0]
        self.tail = (24.0, 32.0)        # the thresholds of the field render and of the per-source kernels
        self.variant, self.parts, self.star = 1, 1, 1

    def refusal(self, name):
        masked = self.nelec == 2
        if name in ("split_traced", "split_cold"):
            return "masked_unhonoured" if masked and not self.honour else None
        if name == "flux":
            if masked and not self.honour:
                return "masked_unhonoured"
            return None if self.split else "no_split"
        if name in SAMPLERS or name in EXACT or name == "pll_isolated":
            if masked:
                return "masked_sampler"
            if name in EXACT and self.window != WINDOWS[0]:
                return "window"
            return None if self.split else "no_split"
        if name == "pll":
            return None if self.split else "no_split"
        if name == "grad":              # (cel_loglik_grad: no row window)
            return "window" if self.window != WINDOWS[0] else None
        return None


def ops(seed, steps, flavour):
    """-> a list of at least `steps` operations (the last group of calls that belong together is finished), each a
    dict(op=, seed=, expect= None or one of REFUSALS, ...)"""
    rnd = random.Random("%s/%d" % (flavour, seed))
    weights = FLAVOURS[flavour]
    names, w = list(weights), [weights[k] for k in weights]
    st = _Abstract()
    out = []
    count = dict.fromkeys(required(flavour), 0)
    backlog = list(PATTERNS) * 2 + list(PROBES)
    if flavour in ("strips", "options"):
        backlog = ["pattern_dirty", "pattern_ready", "probe_window", "probe_no_split"] + list(INPUT_PATTERNS)
    elif flavour == "stars":            # (no masked pixels, no galaxies, no exact conditional: the star-only kernels' walk)
        backlog = ["pattern_dirty", "pattern_ready", "pattern_tail_split"]
    OPT = {"opt_incremental": "inc", "opt_split_reuse": "reuse", "opt_honour_mask": "honour", "opt_split_full_box": "full", "opt_kernel": "variant",
           "opt_tile_parts": "parts", "opt_star_tiles": "star"}
    samplers = SAMPLERS if flavour != "stars" else ("flux", "slice_locations")

    def emit(name, **kw):
        expect = kw.pop("expect", None) or st.refusal(name)
        op = dict(op=name, seed=rnd.randrange(1, 1 << 30), expect=expect, **kw)
        if mark:
            op["pattern"] = mark.pop()
        if name == "mass":          # (would the short cut be taken: the split's sums of this very catalogue, and the options still say so)
            op["ready"] = bool(st.split and st.split["sums"] and not st.split["dirty"] and st.reuse == 2 and not st.full and st.split["tail"] == st.tail[1])
        out.append(op)
        if name in count:
            count[name] += 1
        if expect is None:
            if name in SET_ROWS or name == "set" or name in SAMPLERS or name in EXACT:
                if st.split:
                    st.split["dirty"] = True
            if name in ("split_traced", "split_cold"):
                st.split = dict(full=bool(st.full), dirty=False, sums=name == "split_traced" and st.reuse == 2 and not st.full and st.nelec != 2,
                                tail=st.tail[1])
            elif name == "set_nelec":
                st.nelec, st.split = kw["kind"], None
            elif name == "opt_tail":
                st.tail = tail_of(st.tail, kw["value"])
            elif name in OPT:
                setattr(st, OPT[name], kw["value"])
            elif name == "window_to" and kw["window"] != st.window:      # (the window it has drops nothing)
                st.window, st.split = kw["window"], None                # a new window leaves no resident split
            elif name == "noise_rows":
                st.noise = kw["rows"]
        return op

    used = {}

    def pick(name, values):
        """one of `values`, the least used so far first: every value of an input comes up in a walk"""
        values = list(values)
        least = min(used.get((name, v), 0) for v in values)
        v = rnd.choice([v for v in values if used.get((name, v), 0) == least])
        used[(name, v)] = least + 1
        return v

    def begin(pattern):
        """the first operation of a named pattern carries its name (coverage counts them)"""
        mark.append(pattern)

    mark = []

    def split(kind=None):
        kind = kind or rnd.choice(("split_traced", "split_cold"))
        emit("render" if kind == "split_traced" else "set_rows_1", **({"loglik": True} if kind == "split_traced" else {}))
        emit(kind)

    def unmask():
        if st.nelec == 2:
            emit("set_nelec", kind=rnd.choice((0, 1)))

    def acceptable(name):
        """the calls that make `name` an accepted call from here"""
        if name == "flux" and st.nelec == 2 and rnd.random() < 0.5:
            if not st.honour:
                emit("opt_honour_mask", value=1)
        elif st.nelec == 2:
            unmask()
        if name in EXACT and not (st.split and st.split["full"]):
            if not st.full:
                emit("opt_split_full_box", value=1)
            split()
        elif not st.split:
            split()

    def ready_options():
        unmask()
        if st.reuse != 2:
            emit("opt_split_reuse", value=2)
        if st.full:
            emit("opt_split_full_box", value=0)

    def one(name):
        if name == "mass_end":              # (never without its _begin)
            name = "mass_begin"
        if st.variant == 0 and name not in DIRECT_OK:
            emit("opt_kernel", value=1)
        if name in SAMPLERS or name in EXACT or name in ("pll", "pll_isolated"):
            if name in EXACT or rnd.random() < 0.8:          # (the exact conditional is asked for only where it is defined)
                acceptable(name)
            emit(name)
        elif name in ("split_traced", "split_cold"):
            split(name)
        elif name == "mass_begin":
            emit("mass_begin")
            if rnd.random() < 0.4:
                emit("set_epsilon")                         # (what the header allows in between)
            emit("mass_end")
        elif name == "set_nelec":
            emit("set_nelec", kind=rnd.choice((0, 1, 2)))
        elif name in OPTIONS:
            was = {"opt_incremental": st.inc, "opt_split_reuse": st.reuse, "opt_honour_mask": st.honour, "opt_split_full_box": st.full}[name]
            emit(name, value=(2 - was) if name == "opt_split_reuse" else (1 - was))
        elif name == "window_to":           # (one time in six the window it has: the no-op, which keeps a resident split)
            emit("window_to", window=st.window if rnd.random() < 1 / 6. else pick(name, [x for x in WINDOWS if x != st.window]))
        elif name == "noise_rows":
            emit("noise_rows", rows=pick(name, NOISE_ROWS))
        elif name == "opt_tail":            # (half the time back to the shipping thresholds: the dirty-tile render and the short cut need two calls at one)
            emit("opt_tail", value="default" if st.tail != (24.0, 32.0) and rnd.random() < 0.5 else pick(name, TAILS))
        elif name == "opt_kernel":          # the direct kernels for a few deterministic readers (its render vouches for no image) ...
            if st.variant:
                emit("opt_kernel", value=0)
                emit("render", loglik=True)
                emit(rnd.choice(("set_rows_1", "set_rows_3")))
                emit(rnd.choice(("render", "render_noll")))
            else:                           # ... and back (the next call of anything else brings the recurrence back as well)
                emit("opt_kernel", value=1)
        elif name == "opt_tile_order":
            emit(name, value=pick(name, (0, 1, 2)))
        elif name == "opt_tile_parts":      # (the dirty-tile render is the one-block-per-tile kernel's: 1 as often as the rest together)
            emit(name, value=1 if st.parts != 1 and rnd.random() < 0.5 else pick(name, (0, 1, 2, 4)))
        elif name == "opt_slice_fuse":
            emit(name, value=pick(name, (0, 2)))
        elif name == "opt_star_tiles":
            emit(name, value=pick(name, (0, 1, 2)))
        elif name == "hand_out":
            # from the hand-out on this set keeps no Poisson partials: its log-likelihood renders every tile.  So it comes in the
            # walk's second half, behind one of each pattern that ends in a dirty-tile render with a log-likelihood
            if len(out) < steps // 2:
                return
            for p in ("pattern_dirty", "pattern_rows_dirty", "pattern_kernel_dirty"):
                if p in backlog:
                    backlog.remove(p)
                    one(p)
            emit("hand_out")
        elif name == "pattern_tail_split":  # a model image of one threshold, the split's totals at another: "cold", like a new sky level
            unmask()
            begin(name)
            emit("render", loglik=True)
            emit("opt_tail", value=rnd.choice([t for t in ("default", "strict", "fast", "all8") if tail_of(st.tail, t)[0] != st.tail[0]]))
            emit("split_cold")
            emit("mass")
        elif name == "pattern_tail_mass":   # the split's stamp sums of one per-source threshold, the masses at another
            ready_options()
            begin(name)
            split("split_traced")
            emit("mass")
            emit("opt_tail", value="source8" if st.tail[1] != 8.0 else "default")
            emit("mass")
            emit("mass_begin")
            emit("mass_end")
        elif name == "pattern_window_split":    # a resident split, another window: every reader of the split refuses, then a new split serves
            s = rnd.choice(SAMPLERS)
            acceptable(s)
            begin(name)
            emit("window_to", window=rnd.choice([w for w in WINDOWS if w != st.window]))
            emit(s)
            emit("mass")
            acceptable(s)
            emit(s)
        elif name == "pattern_rows_dirty":  # other owned rows under the per-tile partials: the dirty-tile render adds the new rows' tiles
            if not st.inc:
                emit("opt_incremental", value=1)
            if st.parts != 1:
                emit("opt_tile_parts", value=1)
            begin(name)
            emit("render", loglik=True)
            emit("noise_rows", rows=rnd.choice([r for r in NOISE_ROWS if r != st.noise]))
            emit(rnd.choice(("set_rows_1", "set_rows_3")))
            emit("render", loglik=True)
        elif name == "pattern_kernel_dirty":    # a render under one variant, then the other, then one changed row
            if not st.inc:
                emit("opt_incremental", value=1)
            if st.parts != 1:
                emit("opt_tile_parts", value=1)
            begin(name)
            emit("render", loglik=True)
            emit("opt_kernel", value=0)
            emit("set_rows_1")
            emit("render", loglik=True)
            emit("opt_kernel", value=1)
            emit("set_rows_1")
            emit("render", loglik=True)
        elif name == "render":
            emit("render", loglik=True)
        elif name == "pattern_dirty":       # device sampler -> full render -> set_rows -> render: the dirty-tile path, if it is legal
            if not st.inc:
                emit("opt_incremental", value=1)
            if st.parts != 1:
                emit("opt_tile_parts", value=1)
            if flavour == "stars" and st.star != 0:     # (neither star-only kernel leaves a base for the dirty-tile render)
                emit("opt_star_tiles", value=0)
            s = rnd.choice(samplers)
            acceptable(s)
            emit(s)
            emit("render", loglik=True)
            emit(rnd.choice(("set_rows_1", "set_rows_3")))
            emit("render", loglik=True)
        elif name == "pattern_ready":       # the mass short cut right behind a traced split ...
            ready_options()
            split("split_traced")
            emit("mass")
            emit(rnd.choice(samplers))      # ... and not behind a sampler's rewrite
            emit("mass")
        elif name == "pattern_end_rebuilt":
            s = rnd.choice(SAMPLERS)
            acceptable(s)
            emit("mass_begin")
            emit(s)
            emit("mass_end", expect="end_rebuilt")
        elif name == "pattern_eps":         # a new sky level under a model image that is on the device: neither the dirty-tile render
            if not st.inc:                  # (which asks for no log-likelihood here: the Poisson partials are not what stops it) ...
                emit("opt_incremental", value=1)
            emit("render", loglik=True)
            emit("set_epsilon")
            emit(rnd.choice(("set_rows_1", "set_rows_3")))
            emit("render_noll")
            emit("render", loglik=True)     # ... nor the split's totals may take the old image: "cold", by the documented rule
            emit("set_epsilon")
            emit("split_cold")
        elif name == "probe_no_split":
            emit("set_nelec", kind=rnd.choice((0, 1)))
            emit(rnd.choice(SAMPLERS + ("pll",)))
        elif name == "probe_masked_unhonoured":
            if st.honour:
                emit("opt_honour_mask", value=0)
            emit("set_nelec", kind=2)
            split()
            emit("flux")
        elif name == "probe_masked_sampler":
            if st.nelec != 2:
                emit("set_nelec", kind=2)
            emit(rnd.choice(SAMPLERS[1:] + ("pll_isolated",)))
        elif name == "probe_window":
            acceptable("exact_slice0")
            emit("window_to", window=WINDOWS[1])
            emit(rnd.choice(EXACT))
            emit("window_to", window=WINDOWS[0])
        else:
            emit(name)

    while len(out) < steps:
        short = [k for k in count if count[k] < NEED]
        left = steps - len(out)
        owed = 6 * len(backlog) + 2 * sum(NEED - count[k] for k in short)       # (roughly the steps still owed to the coverage)
        forced = rnd.random() < max(0.15, owed / float(left))
        if forced and backlog and (not short or rnd.random() < 0.3):
            one(backlog.pop(rnd.randrange(len(backlog))))
        elif forced and short:
            one(rnd.choice(short))
        else:
            one(rnd.choices(names, w)[0])
    return out


def coverage(seq, flavour="gibbs"):
    """what a sequence of ops() holds: counts per operation the flavour owes, per expected refusal, per named pattern; and whether
    every mass_end has its mass_begin"""
    count = dict.fromkeys(required(flavour), 0)
    refused = dict.fromkeys(REFUSALS, 0)
    pat = dict(dirty=0, ready=0, not_ready=0, end_rebuilt=0, eps_render=0, eps_split=0)
    if flavour in ("strips", "options"):
        pat = dict(dict.fromkeys(INPUT_PATTERNS, 0), dirty=0, ready=0, not_ready=0)
    pending, paired, stage = False, True, 0
    for i, op in enumerate(seq):
        n = op["op"]
        if n in count:
            count[n] += 1
        if op["expect"]:
            refused[op["expect"]] += 1
        if op.get("pattern") in pat:
            pat[op["pattern"]] += 1
        if n == "mass_begin":
            pending = True
        elif n == "mass_end":
            paired, pending = paired and pending, False
            if "end_rebuilt" in pat:
                pat["end_rebuilt"] += op["expect"] == "end_rebuilt"
        elif n == "mass":
            pat["ready" if op["ready"] else "not_ready"] += 1
        last = [o["op"] for o in seq[max(i - 3, 0):i]]
        if n == "render_noll" and last[-3:-1] == ["render", "set_epsilon"] and last[-1] in SET_ROWS[:3] and "eps_render" in pat:
            pat["eps_render"] += 1
        if n == "split_cold" and last[-2:] == ["render", "set_epsilon"] and "eps_split" in pat:
            pat["eps_split"] += 1
        # device sampler -> render -> set_rows -> render
        ok = not op["expect"]
        if n in SAMPLERS and ok:
            stage = 1
        elif n in ("render", "render_noll") and stage in (1, 3):
            pat["dirty"] += stage == 3
            stage = 2 if stage == 1 else 0
        elif n in SET_ROWS[:3] and stage == 2:
            stage = 3
        else:
            stage = 0
    return count, refused, pat, paired


# ---- the scene ---------------------------------------------------------------------------------------------------------------------
H, W, B, S = 192, 160, 2, 40            # 3 x 5 render tiles of 64 rows x 32 columns per band: interior tiles, border tiles, boxes over several
T2, OFF, CORNER, THIN, FAINT = 0, (1, 2), 3, 4, 5
SIGMA_LOC, SIGMA_STEP, SIGMA_SHAPE = 1e-3, 2e-4, 0.05     # (degrees, degrees, shape units: the existing slice tests' values)
MAX_STEPS_OUT = 8                        # a source without a photon has a flat conditional: the doubling ends here
REFUSAL_TEXT = ("masked", "resident photon split", "row window", "rebuilt since", "without a cel_stamp_mass_begin")
_scene = {}


def scene(cel, stars_only=False):
    """the walk's frame and catalogue (made once): 2 bands, 192 x 160, 40 sources -- 24 stars, 15 type-1 galaxies and ONE type-2
    galaxy, which no sampler turns into anything else: n_gal >= 1 on the live pair and on every replay, so both take the general
    kernel.  Two sources are off the frame, one star sits in a corner, one galaxy is thinner than k_prep's floor, one is fainter
    than eps / 16 in one band (the mass short cut's left-over list).  nelec is drawn once from the model; three images of it:
    plain, one pixel above 65 535, a few NaNs.   stars_only: 12 stars on the same frame (the star-only kernels' scene)"""
    if stars_only in _scene:
        return _scene[stars_only]
    import numpy as np
    from desi_mcmc_amd import synth
    rs = np.random.RandomState(77 if stars_only else 5)
    n = 12 if stars_only else S
    bands = synth.make_bands(H, W, B)
    pix = np.column_stack([rs.uniform(6, W - 6, n), rs.uniform(6, H - 6, n)])
    typ = np.zeros(n, dtype=np.int32)
    shape = np.zeros((n, 4))
    counts = np.exp(rs.uniform(np.log(1.0), np.log(100.0), (n, B))) / bands[None, :, 2] * bands[None, :, 1]
    if not stars_only:
        gal = [OFF[1], THIN, FAINT] + list(range(26, 38))
        typ[gal] = 1
        shape[gal] = np.column_stack([rs.uniform(0.05, 0.95, 15), np.exp(rs.uniform(np.log(0.5), np.log(3.0), 15)), rs.uniform(0, 180, 15),
                                      rs.uniform(0.2, 0.95, 15)])
        typ[T2], shape[T2] = 2, (0.5, 4.0, 0.0, 4.0)                # (theta, W00, W01, W11), pixels^2
        pix[OFF[0]], pix[OFF[1]] = (-500.0, 80.0), (W + 400.0, 50.0)
        pix[CORNER] = (1.5, 2.0)
        shape[THIN, 1] = 0.02                                       # below the 1/30 floor
        counts[FAINT, 1] = bands[1, 0] / 40.0                       # < eps / 16
    radec = synth.pixel2equa(bands[0], pix)
    ctx = cel.Context(0)
    im = cel.ImageSet(ctx, bands, H, W)
    im.render(cel.SourceSet(ctx, n, B).set(typ, radec, counts, shape))
    plain = rs.poisson(im.model_images()).astype(np.float64)
    im.close()
    k = int(np.argmax(counts[26:38, 0])) + 26 if not stars_only else 0
    px, py = int(pix[k, 0]), int(pix[k, 1])
    wide = plain.copy()
    wide[1, py, px] = 70000.0                                       # (on a bright source: photons to split)
    holes = plain.copy()
    yy, xx = rs.randint(0, H, 40), rs.randint(0, W, 40)
    holes[rs.randint(0, B, 40), yy, xx] = np.nan
    if not stars_only:                                              # ... some of them on a bright source
        holes[0, py - 1:py + 2, px] = np.nan
    _scene[stars_only] = dict(bands=bands, cat=(typ, radec, counts, shape), nelec=(plain, wide, holes), n=n)
    return _scene[stars_only]


# ---- the walker ------------------------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


class Walker(object):
    def __init__(self, cel, stars_only=False, required=OPERATIONS):
        import numpy as np
        self.np, self.cel, self.L = np, cel, cel._lib
        sc = scene(cel, stars_only)
        self.sc, self.n = sc, sc["n"]
        self.ctx = cel.Context(0)
        self.ctx.set_option(self.L.CEL_OPT_TILE_PARTS, 1)           # (the dirty-tile path is the one-wave-per-tile kernel's)
        L = self.L
        self.keys = dict(inc=L.CEL_OPT_INCREMENTAL, reuse=L.CEL_OPT_SPLIT_REUSE, honour=L.CEL_OPT_HONOUR_MASK, full=L.CEL_OPT_SPLIT_FULL_BOX,
                         lists=L.CEL_OPT_PHOTON_LISTS, render_T=L.CEL_OPT_TAIL_LOG, tail_T=L.CEL_OPT_TAIL_LOG_SOURCE, variant=L.CEL_OPT_KERNEL,
                         parts=L.CEL_OPT_TILE_PARTS, star=L.CEL_OPT_STAR_TILES, order=L.CEL_OPT_TILE_ORDER, fuse=L.CEL_OPT_SLICE_FUSE)
        self.opt = {k: self.ctx.get_option(v) for k, v in self.keys.items()}
        self.noise = NOISE_ROWS[0]
        self.cur = [np.array(a, copy=True) for a in sc["cat"]]
        self.eps = sc["bands"][:, 0].copy()
        self.kind = 0
        self.im = cel.ImageSet(self.ctx, sc["bands"], H, W, nelec=sc["nelec"][0])
        self.ss = cel.SourceSet(self.ctx, self.n, B).set(*self.cur)
        self.split = None               # dict(cat, seed, traced, opt, eps, dirty) of the live pair's resident split
        self.window = WINDOWS[0]
        self.log = []
        self.count = dict.fromkeys(required, 0)
        self.refused = dict.fromkeys(REFUSALS, 0)
        self.seen = dict(ready1=0, ready0=0, dirty_after_pattern=0, dirty=0, full=0, sampler_ok=0)
        self.stage = 0
        self.letters, self.calib, self.kappa = [0, 1], sc["bands"][:, 2].copy(), sc["bands"][:, 1].copy()

    # -- fresh objects ---------------------------------------------------------------------------------------------------------
    def bands(self, eps):
        b = self.sc["bands"].copy()
        b[:, 0] = eps
        return b

    def fresh(self, cat, eps=None, pixels=None):
        """a pair without memory: today's window and owned rows FIRST, before any call"""
        im = self.cel.ImageSet(self.ctx, self.bands(self.eps if eps is None else eps), H, W, nelec=self.sc["nelec"][self.kind] if pixels is None else pixels)
        if self.window != WINDOWS[0]:
            im.set_window(*self.window)
        if self.noise != NOISE_ROWS[0]:
            im.set_noise_rows(*self.noise)
        return im, self.cel.SourceSet(self.ctx, self.n, B).set(*cat)

    def options(self, want):
        """set the options `want` now -> what they were"""
        was = dict(self.opt)
        want = dict(want)
        T = (want.pop("render_T", self.opt["render_T"]), want.pop("tail_T", self.opt["tail_T"]))
        if T != (self.opt["render_T"], self.opt["tail_T"]):         # (CEL_OPT_TAIL_LOG sets both, CEL_OPT_TAIL_LOG_SOURCE the second)
            self.ctx.set_option(self.keys["render_T"], T[0])
            self.ctx.set_option(self.keys["tail_T"], T[1])
            self.opt["render_T"], self.opt["tail_T"] = T
        for k, v in want.items():
            if self.opt[k] != v:
                self.ctx.set_option(self.keys[k], v)
                self.opt[k] = v
        return was

    def time_options(self):
        """what a resident split remembers of the options: everything that changes a bit of it -- thresholds, variant, and the
        blocks per tile / the star-tile kernel of the render behind its totals (values "agree to rounding between settings",
        include/celeste_hip.h) -- and not what never changes a result (tile order, slice fuse: the replay runs under today's)"""
        return {k: v for k, v in self.opt.items() if k not in ("order", "fuse")}

    def with_split(self, eps=None):
        """a fresh pair brought to the live pair's state the documented way: the catalogue of the split, the options of the
        split, the trace render if there was one, the split with its seed; then today's options, sky levels and catalogue (only if
        it changed: an unchanged one keeps the mass short cut on both sides).  Window and owned rows are today's from the start: a
        split of another window does not exist (cel_images_set_window drops it)"""
        sp = self.split
        if sp is None:
            im, ss = self.fresh(self.cur, eps)
        else:
            im, ss = self.fresh(sp["cat"], sp["eps"])
            now = self.options(sp["opt"])
            try:
                if sp["traced"]:
                    im.render(ss, loglik=True)
                im.photon_split_resident(ss, sp["seed"])
            finally:
                self.options(now)
            eps = self.eps if eps is None else eps
            for b in range(B):
                if sp["eps"][b] != eps[b]:
                    im.set_epsilon(b, eps[b])
            if sp["dirty"]:
                ss.set(*self.cur)
        return im, ss

    # -- comparisons -------------------------------------------------------------------------------------------------------------
    def fail(self, what):
        raise Mismatch("step %d: %s\n   last operations: %s\n   options %s, pixels %d, split %s" % (
            len(self.log), what, self.log[-14:], self.opt, self.kind,
            None if self.split is None else {k: self.split[k] for k in ("seed", "traced", "opt", "dirty")})
            + "\n   window %s, owned rows %s" % (self.window, self.noise))

    def same(self, what, a, b):
        """bit for bit (a NaN where a source was left alone equals a NaN)"""
        np = self.np
        if isinstance(a, dict):
            for k in a:
                self.same("%s[%r]" % (what, k), a[k], b[k])
            return
        if isinstance(a, (tuple, list)):
            if len(a) != len(b):
                self.fail("%s: %d values against %d" % (what, len(a), len(b)))
            for i, (x, y) in enumerate(zip(a, b)):
                self.same("%s[%d]" % (what, i), x, y)
            return
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape or a.dtype != b.dtype:
            self.fail("%s: %s %s against %s %s" % (what, a.dtype, a.shape, b.dtype, b.shape))
        if a.dtype == np.float64:
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            bad = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))
        else:
            bad = a != b
        if np.any(bad):
            idx = np.argwhere(bad)
            a_, b_ = a[bad], b[bad]
            with np.errstate(all="ignore"):
                rel = np.nanmax(np.abs(a_.astype(np.float64) - b_) / np.maximum(np.abs(b_.astype(np.float64)), 1e-300))
            self.fail("%s differs from the replay in %d of %d values (first at %s: %r against %r; largest relative difference %.3e)"
                      % (what, idx.shape[0], a.size, idx[0].tolist(), a_[0], b_[0], rel))

    def outcome(self, call):
        """-> ("ok", values) or ("error", exception class name, message)"""
        try:
            return ("ok", call())
        except Exception as e:                      # (compared with the replay's, never swallowed)
            return ("error", "ValueError" if isinstance(e, ValueError) else type(e).__name__, str(e))

    def both(self, name, expect, live, replay, sampler=False, eps=None):
        """the same call on the live pair and on the replay: both refused where the documentation refuses, equal otherwise (a
        failure that depends on the data -- a chain outside its own conditional -- must be the same failure); afterwards the two
        catalogues are equal in all four arrays"""
        info = (self.im.masked.copy(), self.samples_info(self.im))
        a = self.outcome(live)
        rim, rss = self.with_split(eps)
        b = self.outcome(lambda: replay(rim, rss))
        refusal = a[0] == "error" and a[1] == "ValueError" and any(t in a[2] for t in REFUSAL_TEXT)
        if expect:
            if not refusal:
                self.fail("%s must be refused (%s) on the live pair: %r" % (name, expect, a[:3] if a[0] == "error" else "accepted"))
            if not (b[0] == "error" and b[1] == "ValueError"):
                self.fail("%s must be refused (%s) on the replay: %r" % (name, expect, b[:3] if b[0] == "error" else "accepted"))
            self.refused[expect] += 1
            self.same("catalogue behind the refused %s" % name, self.ss.get(), tuple(self.cur))
            self.same("split behind the refused %s" % name, info, (self.im.masked.copy(), self.samples_info(self.im)))
        else:
            if refusal:
                self.fail("%s refused on the live pair: %s" % (name, a[2]))
            if a[0] != b[0] or (a[0] == "error" and a[1:] != b[1:]):
                self.fail("%s: live %r, replay %r" % (name, a[:3] if a[0] == "error" else "ok", b[:3] if b[0] == "error" else "ok"))
            if a[0] == "ok":
                self.same(name, a[1], b[1])
            if sampler:
                self.cur = [x.copy() for x in self.ss.get()]
                if self.split:
                    self.split["dirty"] = True
                self.seen["sampler_ok"] += 1
        self.same("catalogue behind %s" % name, self.ss.get(), rss.get())
        rim.close()
        return a

    def samples_info(self, im):
        import ctypes as C
        s, tot = C.c_int64(0), C.c_int64(0)
        self.L.check(self.L.lib().cel_samples_info(im._h, C.byref(s), C.byref(tot)))
        return (s.value, tot.value)

    # -- host edits (tools/dbg/incremental_stress.py's kinds) -------------------------------------------------------------------
    def edit(self, rows, rs):
        """every edit changes its row by at least 1e-3 relative or 0.05 pixel (5.5e-6 degrees): a stale answer misses by orders
        of magnitude, not by rounding"""
        np, cur, bands = self.np, self.cur, self.sc["bands"]
        from desi_mcmc_amd import synth
        for s in rows:
            what = rs.randint(6)
            if what == 3 and (cur[0][s] == 2 or self.n != S):
                what = 4
            if what == 5 and cur[0][s] != 1:
                what = 0
            if what == 0:                   # a sub-pixel move
                d = rs.normal(0, 2e-5, 2)
                cur[1][s] += d + np.sign(d) * 6e-6
            elif what == 1:                 # across the frame (or back onto it)
                cur[1][s] = synth.pixel2equa(bands[0], np.array([[rs.uniform(-20, W + 20), rs.uniform(-20, H + 20)]]))[0]
            elif what == 2:                 # off the frame
                cur[1][s] = synth.pixel2equa(bands[0], np.array([[-500.0 - rs.uniform(0, 100), rs.uniform(0, H)]]))[0]
            elif what == 3:                 # star <-> galaxy
                cur[0][s] = 1 - cur[0][s]
                cur[3][s] = [rs.uniform(0.05, 0.95), np.exp(rs.uniform(np.log(0.3), np.log(3.0))), rs.uniform(0, 180), rs.uniform(0.2, 1.0)] \
                    if cur[0][s] == 1 else [0, 0, 0, 0]
            elif what == 4:                 # fluxes
                g = rs.normal(0, 0.5, B)
                cur[2][s] *= np.exp(g + np.sign(g) * 2e-3)
            else:                           # sigma
                g = rs.normal(0, 0.3)
                cur[3][s, 1] *= np.exp(g + np.sign(g) * 2e-3)

    def touched(self):
        if self.split:
            self.split["dirty"] = True

    # -- one operation -------------------------------------------------------------------------------------------------------------
    def run(self, op):
        np, name, expect = self.np, op["op"], op.get("expect")
        rs = np.random.RandomState(op["seed"])
        n = self.n
        note = name
        stage, self.stage = self.stage, 0
        self.log.append(name + ("!" + expect if expect else ""))            # (a failure names the call it happened in)
        if name in SET_ROWS:
            k = min(int(name.split("_")[-1]), n)
            rows = rs.choice(n, k, replace=False).astype(np.int32)
            self.edit(rows, rs)
            self.ss.set_rows(rows, *[a[rows] for a in self.cur])
            self.touched()
            self.stage = 3 if (stage == 2 and k <= 20) else 0
        elif name == "set":
            g = rs.normal(0, 0.05, self.cur[2].shape)
            self.cur[2] = self.cur[2] * np.exp(g + np.sign(g) * 2e-3)
            self.ss.set(*self.cur)
            self.touched()
        elif name in ("render", "render_noll"):
            loglik = name == "render"
            out = self.im.render(self.ss, loglik=loglik)
            d = self.im.last_render_dirty_tiles()
            rim, rss = self.fresh(self.cur)
            want = rim.render(rss, loglik=loglik)
            self.same("render: model images (dirty tiles %d)" % d, self.im.model_images(), rim.model_images())
            if loglik:
                self.same("render: log-likelihood (dirty tiles %d)" % d, out, want)
                self.same("render: stats", self.im.stats(), rim.stats())
            rim.close()
            self.seen["dirty" if d >= 0 else "full"] += 1
            if stage == 3 and d >= 0:
                self.seen["dirty_after_pattern"] += 1
            self.stage = 2 if (stage == 1 and d < 0) else 0
            note = "%s->%d" % (name, d)
        elif name in ("split_traced", "split_cold"):
            # (the generator put render(loglik=True) / a set_rows edit immediately before: both sides form the totals image by
            # the documented rule of CEL_OPT_SPLIT_REUSE)
            seed = op["seed"]
            sp = dict(cat=[a.copy() for a in self.cur], seed=seed, traced=name == "split_traced", opt=self.time_options(), eps=self.eps.copy(), dirty=False)

            def values(im, noise):
                return dict(noise=noise, sums=im.sample_sums(), samples=im.fetch_samples(), rects=im.photon_rects(), rates=im.split_rates(),
                            info=self.samples_info(im))

            a = self.outcome(lambda: values(self.im, self.im.photon_split_resident(self.ss, seed)))
            rim, rss = self.fresh(self.cur)
            b = self.outcome(lambda: values(rim, (rim.render(rss, loglik=True) if sp["traced"] else None, rim.photon_split_resident(rss, seed))[1]))
            if expect:
                if not (a[0] == "error" and a[1] == "ValueError" and "masked" in a[2]) or b[:2] != ("error", "ValueError"):
                    self.fail("%s must be refused (%s): live %r, replay %r" % (name, expect, a[:3] if a[0] == "error" else "accepted", b[:3] if b[0] == "error" else "accepted"))
                self.refused[expect] += 1
            else:
                if a[0] != "ok" or b[0] != "ok":
                    self.fail("%s: live %r, replay %r" % (name, a, b))
                self.same(name, a[1], b[1])
                self.split = sp
            rim.close()
        elif name == "mass":
            ready = self.im.stamp_mass_ready(self.ss)
            self.seen["ready1" if ready else "ready0"] += 1
            a = self.both("mass", None, lambda: (self.im.stamp_mass_ready(self.ss), self.im.stamp_mass(self.ss)),
                          lambda im, ss: (im.stamp_mass_ready(ss), im.stamp_mass(ss)))
            self.third_mass("mass", a[1][1], exact=not ready)
            note = "mass(ready=%d)" % ready
        elif name == "mass_begin":
            self.im.stamp_mass_begin(self.ss)
            self.begin_eps = self.eps.copy()
        elif name == "mass_end":
            def replay(im, ss):
                im.stamp_mass_begin(ss)
                if expect:              # what a sampler in between does to the pending call: a new generation, its records rebuilt
                    ss.set(*self.cur)
                    im.source_boxes(ss)
                return im.stamp_mass_end()
            # (the short cut's left-over list is drawn up by _begin, at the sky levels of that moment)
            a = self.both("mass_end", expect, lambda: self.im.stamp_mass_end(), replay, eps=None if expect else self.begin_eps)
            if not expect:
                self.third_mass("mass_end", a[1])
        elif name == "flux":
            fs = op["seed"]
            a = self.both("flux", expect, lambda: self.im.flux_conditionals(self.ss, fs, 5.0, 0.005, self.letters, self.calib, self.kappa),
                          lambda im, ss: im.flux_conditionals(ss, fs, 5.0, 0.005, self.letters, self.calib, self.kappa), sampler=True)
            if not expect and a[0] == "ok":
                self.stage = 1
        elif name in SAMPLERS or name in EXACT:
            ids = np.arange(n, dtype=np.int32)
            ids[rs.rand(n) < 0.2] = -1                      # (a dealt chain: these sources are somebody else's)
            sd = op["seed"]
            cond = "exact" if name in EXACT else "reference"
            if name == "slice_locations":
                call = lambda im, ss: im.slice_locations(ss, SIGMA_LOC, sd, chain_ids=ids)
            elif name in ("slice_sample0_comp", "exact_slice0"):
                so = bool(rs.randint(2)) if name != "exact_slice0" else False
                call = lambda im, ss: im.slice_sample(ss, 0, SIGMA_STEP if so else SIGMA_LOC, sd, step_out=so, max_steps_out=MAX_STEPS_OUT,
                                                      chain_ids=ids, conditional=cond)
            elif name == "slice_sample0_dirs":
                dirs = rs.normal(size=(n, 2, 2))
                dirs /= np.sqrt((dirs ** 2).sum(axis=2, keepdims=True))
                so = bool(rs.randint(2))
                call = lambda im, ss: im.slice_sample(ss, 0, SIGMA_STEP if so else SIGMA_LOC, sd, dirs=dirs, step_out=so, max_steps_out=MAX_STEPS_OUT,
                                                      chain_ids=ids)
            elif name in ("slice_sample1", "exact_slice1"):
                phi_max = 180.0 if rs.randint(2) else 0.0
                call = lambda im, ss: im.slice_sample(ss, 1, SIGMA_SHAPE, sd, step_out=bool(phi_max), max_steps_out=MAX_STEPS_OUT, phi_max=phi_max,
                                                      chain_ids=ids, conditional=cond)
            else:
                shapes = np.column_stack([rs.uniform(0.05, 0.95, n), np.exp(rs.uniform(np.log(0.3), np.log(3.0), n)), rs.uniform(0, 180, n),
                                          rs.uniform(0.2, 0.95, n)])
                h = op.get("h", rs.choice([-30.0, 0.0, 30.0], n) + rs.normal(0, 3, n))
                call = lambda im, ss: im.type_move(ss, shapes, h, sd, chain_ids=ids, conditional=cond)
            a = self.both(name, expect, lambda: call(self.im, self.ss), call, sampler=True)
            if not expect and a[0] == "ok" and name in SAMPLERS:
                self.stage = 1
        elif name in ("pll", "pll_isolated"):
            P = 8
            own = rs.choice(n, P, replace=False).astype(np.int32)
            prop = [self.cur[0][own], self.cur[1][own] + rs.normal(0, 1e-5, (P, 2)), self.cur[2][own], self.cur[3][own]]
            iso = name == "pll_isolated"
            call = lambda im, ss: im.patch_loglik_resident(self.cel.SourceSet(self.ctx, P, B).set(*prop), own, isolated=iso)
            self.both(name, expect, lambda: call(self.im, self.ss), call)
        elif name == "estep":
            rim, rss = self.fresh(self.cur)
            self.same("estep", self.im.estep_stats(self.ss), rim.estep_stats(rss))
            rim.close()
        elif name == "grad":
            rim, rss = self.fresh(self.cur)
            a, b = self.outcome(lambda: self.im.loglik_grad(self.ss)), self.outcome(lambda: rim.loglik_grad(rss))
            if expect:
                if not (a[0] == "error" and a[1] == "ValueError" and "row window" in a[2]) or b[:2] != ("error", "ValueError"):
                    self.fail("grad must be refused (%s): live %r, replay %r" % (expect, a[:3] if a[0] == "error" else "accepted", b[:3] if b[0] == "error" else "accepted"))
                self.refused[expect] += 1
            else:
                if a[0] != "ok" or b[0] != "ok":
                    self.fail("loglik_grad: live %r, replay %r" % (a[:3], b[:3]))
                self.same("loglik_grad", a[1], b[1])
            rim.close()
        elif name == "set_epsilon":
            b = int(rs.randint(B))
            self.eps[b] = self.sc["bands"][b, 0] * (1 + 1e-2 * (0.1 + rs.rand()))
            self.im.set_epsilon(b, self.eps[b])
        elif name == "set_nelec":
            self.kind = op["kind"]
            self.im.set_nelec(self.sc["nelec"][self.kind])
            self.split = None                                   # new pixels drop the resident split (include/celeste_hip.h)
            self.same("cel_samples_info behind set_nelec", self.samples_info(self.im), (0, 0))
            self.same("stamp_mass_ready behind set_nelec", self.im.stamp_mass_ready(self.ss), False)
            note = "set_nelec(%d)" % self.kind
        elif name == "opt_tail":
            T = tail_of((self.opt["render_T"], self.opt["tail_T"]), op["value"])
            if op["value"] in ("default", "strict", "fast"):    # (the presets go the way a caller's do)
                self.ctx.set_tail_log(op["value"])
                self.opt["render_T"], self.opt["tail_T"] = T
            else:
                self.options(dict(render_T=T[0], tail_T=T[1]))
            self.same("the thresholds behind opt_tail", (self.ctx.get_option(self.keys["render_T"]), self.ctx.get_option(self.keys["tail_T"])), T)
            note = "opt_tail=%s" % op["value"]
        elif name.startswith("opt_"):
            key = {"opt_incremental": "inc", "opt_split_reuse": "reuse", "opt_honour_mask": "honour", "opt_split_full_box": "full", "opt_kernel": "variant",
                   "opt_tile_order": "order", "opt_tile_parts": "parts", "opt_slice_fuse": "fuse", "opt_star_tiles": "star"}[name]
            self.options({key: float(op["value"])})
            note = "%s=%d" % (name, op["value"])
        elif name == "window_to":
            window = tuple(op["window"])
            info = self.samples_info(self.im)
            self.im.set_window(*window)
            if window != self.window:                           # a new window drops the resident split (include/celeste_hip.h) ...
                self.window, self.split = window, None
                self.same("cel_samples_info behind a new window", self.samples_info(self.im), (0, 0))
                self.same("stamp_mass_ready behind a new window", self.im.stamp_mass_ready(self.ss), False)
            else:                                               # ... the window it has drops nothing
                self.same("cel_samples_info behind the same window", self.samples_info(self.im), info)
            note = "window_to%s" % (window,)
        elif name == "noise_rows":
            self.noise = tuple(op["rows"])
            self.im.set_noise_rows(*self.noise)
            note = "noise_rows%s" % (self.noise,)
        elif name == "hand_out":
            # the observed pixels' address, and the SAME pixels written through it: the numbers stay comparable, and the library
            # has to treat the pixels as the caller's from now on (a resident split stays the split of the pixels it was drawn from)
            self.write_pixels(self.sc["nelec"][self.kind])
        else:
            raise KeyError(name)
        if name in self.count:
            self.count[name] += 1
        self.log[-1] = note + ("!" + expect if expect else "")

    def write_pixels(self, pixels):
        """cel_images_device_ptrs for the observed pixels, and `pixels` copied to that address"""
        import ctypes as C
        np = self.np
        pixels = np.ascontiguousarray(pixels, dtype=np.float64)
        assert pixels.shape == (B, H, W)                        # (the device buffer's size: nothing is written past it)
        hip = C.CDLL(self.L.LIB_PATH)                           # (dlsym through the library finds the HIP runtime IT is linked to)
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.ctx.synchronize()
        if hip.hipMemcpy(self.im.device_ptrs()[0], pixels.ctypes.data, pixels.nbytes, 1) != 0:
            raise RuntimeError("hipMemcpy to the observed pixels failed")

    def third_mass(self, what, got, exact=False):
        """the mass kernel alone, on an object that never had a split: the short cut's bound (CEL_OPT_SPLIT_REUSE: 1.6e-10 at
        the thresholds; tools/dbg/reuse_stress.py's rtol = 1e-9, atol = 1e-15).  That figure is the shipping per-source threshold's,
        T = 32: the sums carry the SPLIT's drop rule (per tile), the mass kernel drops per source, and either leaves out terms
        below eps e^-T -- under a coarser threshold the ceiling of every such term, and with it the bound, is e^(32 - T) times
        higher (measured at T = 20: 8.9e-8 against 1.6e-4).  exact: the live pair did not take the short cut either, so the two
        are the same kernel on the same records -- bit for bit"""
        np = self.np
        im, ss = self.fresh(self.cur)
        want = im.stamp_mass(ss)
        im.close()
        if exact:
            self.same("%s by the mass kernel, against an object without a split" % what, got, want)
        rtol = 1e-9 * max(1.0, float(np.exp(32.0 - self.opt["tail_T"])))
        if not np.allclose(got, want, rtol=rtol, atol=1e-15):
            i = np.unravel_index(int(np.argmax(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))), want.shape)
            self.fail("%s off the mass kernel's values: source %d band %d %r against %r (type %d, counts %r, shape %r)"
                      % (what, i[0], i[1], got[i], want[i], self.cur[0][i[0]], self.cur[2][i[0]].tolist(), self.cur[3][i[0]].tolist()))

    def walk(self, seq):
        for op in seq:
            self.run(op)
        return self

    def close(self):
        self.im.close()
