// celeste_hip.hip -- MI355X (gfx950 / CDNA4) implementation of CelestePy's model-image
// rendering + Poisson log-likelihood path behind the C ABI of include/celeste_hip.h.
//
// Path (reference file:line, relative to the HIPS/DESI-MCMC root):
//   equa2pixel / cd_at_pixel            CelestePy/fits_image.py:166-216
//   calc_bounding_radius                CelestePy/util/bound/bounding_box.py:9-31
//   galaxy transform + MoG (x) MoG      CelestePy/celeste_galaxy_conditionals.py:90-125,185-214
//                                       CelestePy/util/dists/mog.py:75-100
//   mixture evaluation on pixel grids   CelestePy/util/dists/mog.py:5-21,
//                                       CelestePy/util/like/gmm_like_fast.pyx:130-176
//   gen_model_image / celeste_likelihood CelestePy/celeste.py:203-252
//
// Design (DESIGN.md has the long form):
//   k_prep    one thread per (band, source): pixel position, galaxy shape matrix, bounding
//             radius, clipped box -> a 128-byte record + a 16-byte box.
//   k_bin_*   two-level binning (256 x 256 super-tiles, then render tiles) with ballot + prefix
//             popcount compaction: every tile's source list comes out in source order --
//             deterministic, no sort, no atomics on list contents; k_order launches the
//             heaviest tiles first.
//   k_render_hw / k_render
//             one wave per tile (32 x 64 with two component groups per column, or 64 x 32 with
//             one lane per column), coalesced row segments.  Gathers every
//             source of the tile's list into an LDS accumulator tile, then writes
//             lambda = eps + acc ONCE and fuses the Poisson term nelec*log(lambda) - lambda
//             with a wavefront shuffle reduction.  Component tables (K = 3 star, 42 galaxy)
//             are built lane-parallel in LDS from the 128-byte record.  Two evaluators:
//               direct    : exp() per Gaussian-pixel
//               recurrence: along a pixel column a Gaussian obeys g(y+1) = g(y) r(y),
//                           r(y+1) = r(y) q with q = exp(-c): 2 mul + 1 add per
//                           Gaussian-pixel after a per-segment seed; segments are bounded so
//                           that no significant lane ever underflows.
//   k_reduce  fixed-order sum of the per-tile partials -> ll per band (bitwise reproducible).
//   k_stamps  per-source stamps into a packed buffer (same column evaluators, no accumulator).
//   k_gmm     generic N-point evaluator (gmm_like_2d).
//   k_patch_ll / k_estep_* / k_photon_split
//             per-source conditional log-likelihoods, E-step reductions, Gibbs photon split.
// All arithmetic is fp64 on the vector ALU; MFMA is not used (no contraction in this path).

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <memory>
#include <new>
#include <vector>
#include <type_traits>

#include "../../include/celeste_hip.h"
#include "host_buf.h"
#include "field_state.h"

// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// A failing call leaves the function at once -- but asynchronous copies queued earlier in it may still be reading
// a local (a std::vector of staged arguments) or a caller's buffer: the error path drains the device first, so that
// nothing is in flight when those go out of scope.  (Error paths only; scratch_get fails through here as well.)
#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            (void)hipDeviceSynchronize();                                                     \
            return fail(e_ == hipErrorOutOfMemory ? CEL_ERR_NOMEM : CEL_ERR_HIP, "%s: %s (%s:%d)", \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                    \
        }                                                                                     \
    } while (0)

#include "device_common.h"
#include "k_prep_bin.h"
#include "k_bin2.h"
#include "k_render.h"
#include "k_render_hw.h"
#include "k_render_stars.h"
#include "k_small_stars.h"
#include "k_border.h"
#include "k_render_qw.h"
#include "k_mask.h"
#include "k_misc.h"
#include "k_stamp_jac.h"
#include "k_patch_ll.h"
#include "k_slice_gen.h"
#include "k_type_move.h"
#include "k_hmc.h"
#include "k_estep.h"
#include "k_grad.h"
#include "k_patch_grad.h"
#include "k_patch_grad_nz.h"
#include "k_mass_grad.h"
#include "k_split.h"
#include "k_moments.h"
#include "k_slice.h"

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct Prof {
    // a ring of event pairs, created once when profiling is switched on: nothing is allocated inside
    // a timed loop, and finished pairs are read back a few at a time as new ones are handed out
    static const int PAIRS = 1024;
    hipEvent_t *ev = nullptr;   // 2 * PAIRS events; pair i = ev[2i], ev[2i+1]
    int kid[PAIRS];
    int head = 0, count = 0;    // next pair to hand out; pairs handed out and not yet read
    double sum_ms[CEL_K_COUNT] = {0};
    int64_t n[CEL_K_COUNT] = {0};
    unsigned seen[CEL_K_COUNT] = {0};   // launches of each kernel since the reset (level 3 times every fourth)
};

// The context's scratch slots (scratch_get), by purpose.  A slot's contents are dead when the call that took it returns --
// except SCR_VALUES after cel_stamp_mass_begin: the masses WAIT there (im->mass.values) for cel_stamp_mass_end, and none of the calls
// the header allows in between (cel_gamma_streams, cel_samples_fetch, cel_images_set_epsilon) takes that slot.
enum ScratchSlot {
    SCR_PLL_BOXES,    // cel_patch_loglik_multi: the caller's boxes, their photon rectangles, the owners
    SCR_OFFSETS,      // cel_patch_loglik_multi, cel_photon_split: a caller's patch offsets
    SCR_VALUES,       // cel_patch_loglik_multi: the jobs' sums; cel_photon_split: the noise partials; cel_stamp_mass_begin: the masses (PENDING)
    SCR_PATCH_DATA,   // cel_patch_loglik_multi, cel_photon_split: a caller's patch pixels, staged; cel_samples_fetch: sums the split did not form; cel_slice_sample's moments (param 10): the S*B*6 sums (free between a split and a sampler call: the samplers and the resident likelihoods take none of it)
    SCR_TMP_A,        // cel_render_stamps: jobs; cel_estep_stats: xtilde; cel_loglik_grad: sums; cel_patch_loglik_multi (gradient form): the parts' sums; cel_mog_loglike: components; cel_galaxy_mixture_params: inputs
    SCR_TMP_B,        // cel_render_stamps: boxes; cel_estep_stats: masses; cel_loglik_grad: staged gradients; cel_patch_loglik_multi (gradient form): the 7 + B rows; cel_mog_loglike: points; cel_galaxy_mixture_params: outputs
    SCR_TMP_C,        // cel_render_stamps: offsets; cel_estep_stats: per-entry sums; cel_mog_loglike: outputs; cel_flux_conditionals, cel_gamma_streams: inputs + outputs
    SCR_HOST_IO,      // cel_sources_set_rows: the staged rows; cel_render_stamps: the stamps on their way to the host
    SCR_COUNT
};
static_assert(SCR_COUNT == 8, "eight scratch slots");

// The context's pinned mailbox: where the entry points' small readbacks land, at fixed offsets.  The union's words are shared on
// purpose: one call uses them at a time and nothing in the union outlives its call.
union MailShared {
    unsigned long long bin_coarse[2];    // render_impl: coarse cursor, coarse overflow -- behind bin_fine, in the same copy
    int64_t scan_total;                  // cel_photon_split: the total of its patch-layout scan, then of its photon-list scan
    int slice_flags[12];                 // flag slot 0 (11 ints): cel_slice_locations' two job counts, then its even batches; cel_slice_sample's six flags
    struct {
        unsigned long long flags_[3];
        unsigned long long slice_bytes;  // cel_slice_locations' byte counter: over flags [6..7], once the last batch has been read
        double field_stats[2];           // cel_field_stats' pair
    } w;
};
struct Mailbox {
    double ll_band[MAX_BANDS];           // the bands' sums: render_impl, cel_photon_split, cel_estep_stats
    unsigned long long bin_fine[2];      // + 0: fine cursor, fine overflow of the binning pass (render_impl)
    MailShared sh;                       // + 2
    int slice_flags1[12];                // + 8: cel_slice_locations' flag slot 1 (11 ints): its odd batches, the fused rounds' totals
    int mass_todo;                       // + 14: the mass short cut's to-do count, PENDING from cel_stamp_mass_begin to _end
    int unused_[3];
};
static_assert(sizeof(Mailbox) == sizeof(double) * (MAX_BANDS + 16), "the mailbox is MAX_BANDS + 16 doubles");
static_assert(offsetof(Mailbox, bin_fine) == sizeof(double) * MAX_BANDS && offsetof(Mailbox, sh) == sizeof(double) * (MAX_BANDS + 2) &&
              offsetof(MailShared, w.slice_bytes) == sizeof(int) * 6 && offsetof(MailShared, w.field_stats) == sizeof(double) * 4 &&
              offsetof(Mailbox, slice_flags1) == sizeof(double) * (MAX_BANDS + 8) && offsetof(Mailbox, mass_todo) == sizeof(double) * (MAX_BANDS + 14),
              "the mailbox members keep their offsets");
static_assert(offsetof(Mailbox, mass_todo) >= offsetof(Mailbox, slice_flags1) + sizeof(int) * 11 && sizeof(MailShared) <= sizeof(double) * 6,
              "the pending to-do count shares no word: flag slot 1 ends before it, the shared words before flag slot 1");

#ifndef SLICE_FUSE_DEFAULT
#define SLICE_FUSE_DEFAULT 0       // CEL_OPT_SLICE_FUSE: off.  Built and measured in round 6 (cel_slice_locations): no gain at any threshold
#endif
struct cel_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int variant = 1;
    // CEL_OPT_TAIL_LOG.  Two thresholds with different defaults: the FIELD render drops against the sky (24: a skipped
    // component is below eps * 4e-11; the benchmark field's log-likelihood keeps all 16 digits, its kernel takes 13 % less
    // time than at 32), the per-source kernels against the source's own value (32: their outputs feed acceptance ratios
    // and are tested to 1e-11).  Setting the option sets both; CEL_TAIL_LOG in the environment is the initial value of both.
    // (the environment value is held to the option's own range, [0, 300]; anything else is ignored)
    static bool env_tail_ok() { const char *e = getenv("CEL_TAIL_LOG"); return e && atof(e) >= 0.0 && atof(e) <= 300.0; }
    double tail_T = env_tail_ok() ? atof(getenv("CEL_TAIL_LOG")) : 32.0;
    double render_T = env_tail_ok() ? atof(getenv("CEL_TAIL_LOG")) : 24.0;
    int live = 0;               // image sets and source sets of this context that have not been destroyed (cel_ctx_destroy refuses)
    int split_full = 0;         // CEL_OPT_SPLIT_FULL_BOX
    int slice_fuse = SLICE_FUSE_DEFAULT;   // CEL_OPT_SLICE_FUSE
    int honour_mask = 0;        // CEL_OPT_HONOUR_MASK
    int slice_conditional = 0;  // CEL_OPT_SLICE_CONDITIONAL
    int grad_conditional = 0;   // CEL_OPT_GRAD_CONDITIONAL
    int sampler_mask = 0;       // CEL_OPT_SAMPLER_MASK
    int comp_cache = (getenv("CEL_COMP_CACHE") && atoi(getenv("CEL_COMP_CACHE")) == 0) ? 0 : 1;          // CEL_OPT_COMP_CACHE (the env var: the initial value, for A/B runs)
    int incremental = (getenv("CEL_INCREMENTAL") && atoi(getenv("CEL_INCREMENTAL")) == 0) ? 0 : 1;       // CEL_OPT_INCREMENTAL
    int tile_parts = (getenv("CEL_TILE_PARTS") && (atoi(getenv("CEL_TILE_PARTS")) == 1 || atoi(getenv("CEL_TILE_PARTS")) == 2 || atoi(getenv("CEL_TILE_PARTS")) == 4))
                         ? atoi(getenv("CEL_TILE_PARTS")) : 0;       // CEL_OPT_TILE_PARTS (the env var: the initial value, for A/B runs)
    int profile = 0;          // CEL_OPT_PROFILE: 0 off, 1 every kernel, 2 the evaluating kernels only
    int star_tiles = (getenv("CEL_STAR_TILES") && atoi(getenv("CEL_STAR_TILES")) >= 0 && atoi(getenv("CEL_STAR_TILES")) <= 3)
                         ? atoi(getenv("CEL_STAR_TILES")) : 1;       // CEL_OPT_STAR_TILES (the env var: the initial value, for test runs)
    int n_cu = 256;           // compute units of the device (set at creation): the binning pass sizes its blocks by it
    int tile_order = 1;       // 0 = launch k_render tiles in index order, 1 = heaviest first by the last render's measured tile durations (estimate when none), 2 = heaviest first by the estimate only
    int tile_rows = 32;       // rows per render tile (32 or 64), read when an image set is created
    bool tile_timing = false; // diagnostic: k_render stamps each tile's start/end wall clock
    double nz_bias = getenv("CEL_NZ_BIAS") ? atof(getenv("CEL_NZ_BIAS")) : 4.0;   // see k_nz_layout (the env var: experiments only)
    int split_reuse = getenv("CEL_SPLIT_REUSE") ? std::min(std::max(atoi(getenv("CEL_SPLIT_REUSE")), 0), 2) : 2;      // CEL_OPT_SPLIT_REUSE (the env var: the initial value, for A/B runs): 1 = the split's totals from a model image already on the device (k_border.h), 2 = ... and the stamp masses from the split's own sums
    bool mass_reuse_of() const { return split_reuse >= 2; }
    int nz_force = 0;         // CEL_OPT_PHOTON_LISTS: 0 = per patch, whichever is estimated cheaper; 1 = every patch at its photons; 2 = never
    bool grad_nz = false;     // ... its values 4 and 5 (= 0 / 1 for the value): the resident gradient reads the lists too (k_patch_grad_nz.h)
    int debug = 0;            // CEL_OPT_DEBUG: timing-only ablation bits handed to the render kernel (results are wrong when set)
    int tile_layout = 1;      // 0: 64 x tile_rows tiles, one lane per column (k_render)
                              // 1: 32 x 64 tiles, two component groups per column (k_render_hw)
    Prof prof;
    PinnedBuf<Mailbox> mail;    // MAX_BANDS + 16 doubles of pinned host memory for readbacks
    hipEvent_t slice_ev[2] = {nullptr, nullptr};     // cel_slice_locations: one per batch of rounds in flight
    // grow-only device scratch for the small per-call buffers of the stamp / patch-ll entry
    // points (an allocation + free pair per call costs more than the kernels they bracket)
    DevBuf<char> scratch[SCR_COUNT];
};

static int scratch_get(cel_ctx *c, ScratchSlot slot, size_t bytes, void **out) {
    if (bytes == 0) bytes = 8;
    HIP_TRY(c->scratch[slot].grow(bytes, bytes + bytes / 2 + 256, c->stream));
    *out = c->scratch[slot];
    return CEL_OK;
}

struct SourcesDeleter {
    void operator()(cel_sources *s) const { cel_sources_destroy(s); }
};

// (FieldState, field_state.h: whose records, lists, model image and photon split the buffers below hold -- im->rec, im->lists,
// im->model, im->split, im->mass -- and the events that are the only writers of those stamps)
struct cel_images : FieldState {
    cel_ctx *ctx = nullptr;
    int B = 0, H = 0, W = 0;   // H = rows held on the device (the window height)
    int full_H = 0, win_y0 = 0;  // the window is rows [win_y0, win_y0 + H) of a full_H-row frame
    int noise_y0 = 0, noise_y1 = 0x7fffffff;     // window rows whose sky photons cel_photon_split's noise sums count
    int TW = 64, TH = 32, ntx = 0, nty = 0;   // render tile geometry (fixed at creation)
    cel_band hb[MAX_BANDS];
    DevBuf<BandDev> d_bands;
    DevBuf<double> d_nelec, d_lambda, d_partials, d_llband;
    bool have_nelec = false;
    // per-render scratch, grown on demand
    DevBuf<double> d_slabs;          // k_render_hw<, PARTS>: PARTS accumulator slabs per render tile, allocated with the first such launch
    DevBuf<int> d_part_cnt;          // ... and the tiles' arrival counters
    // grown together (ensure_recs: grow_group); d_recs is named last, so its capacity is the group's
    DevBuf<SrcRec> d_recs;
    DevBuf<int4> d_boxes;
    DevBuf<int> d_kind;
    DevBuf<int> d_status;          // per (band, source): 1 has a stamp, 0 empty box, -1 overlap-test miss
    DevBuf<double> d_comps;        // the component cache: COMP_ROW doubles per (band, source) record (k_comps.h; rec.comps_gen), grown on first use
    // the host copy of the boxes / status that cel_stamp_boxes / cel_source_boxes hand out (rec.hbox_gen):
    // a stamp call (boxes, then stamps) runs k_prep and the D2H once, not twice
    DevBuf<unsigned long long> d_massfx;      // the split's integer stamp-mass sums (k_split.h, k_border.h), per (source, band): split.massfx_gen
    DevBuf<int> d_mass_todo;                  // (source, band) jobs the mass kernel proper still has to do + their count behind them
    std::vector<int4> h_boxes;
    std::vector<int> h_status;
    DevBuf<int> d_tile_cnt, d_tile_nstar, d_tile_work, d_order;
    DevBuf<int> d_tile_cost;      // measured duration of every tile in the last render (the next render's launch order)
    bool bin_two_level = false;   // a super-tile once held more than BIN_CH candidates: coarse lists in global memory from then on
    DevBuf<long long> d_btot;        // per-1024-entries totals of the patch / list layout scans
    int64_t masked[MAX_BANDS] = {0}; // NaN (masked) pixels per band that the last cel_images_set_nelec found (cel_images_mask_info)
    bool any_masked = false;         // ... at least one: a MASKED set (k_mask.h, the masked twins of the gradient and E-step kernels)
    bool star_one_segment = false;   // every band passes star_setup's test: k_render_stars may take star tiles
    hipEvent_t ev_step = nullptr; // marks a step's readback copy: the host waits for it, not for the sort queued behind it
    DevBuf<int64_t> d_tile_off;
    unsigned long long *d_cursor = nullptr;   // fine cursor, fine overflow, coarse cursor, coarse overflow (inside d_llband), and the binning
                                              // pass's saved and changed-at words behind them (BIN_WORDS, k_prep_bin.h)
    unsigned long long bin_step = 0;          // renders that asked k_prep to compare its boxes so far: the step number of the next is + 1
    DevBuf<int> d_lists;
    int nsx = 0, nsy = 0;                     // 256 x 256 super-tiles of the coarse binning level
    DevBuf<int> d_sup_cnt;
    DevBuf<int64_t> d_sup_off;
    DevBuf<int> d_clist;
    DevBuf<unsigned long long> d_timing;      // CEL_OPT_TILE_TIMING diagnostic stamps, 3 per tile
    // device-resident sample patches of the last resident photon split (source-major, index s*B+b)
    DevBuf<int> d_samp;         // the resident photon split's sample patches: int32 photon counts, source-major
    // host copies of the last resident split's sums and patch offsets (pinned), made INSIDE cel_photon_split before its last
    // wait: cel_samples_fetch hands them over without touching the stream, on which the photon lists are still being compacted
    // (grown together; h_ssum is named last, so its capacity is the pair's)
    PinnedBuf<double> h_ssum;
    PinnedBuf<int64_t> h_soff;
    DevBuf<NzEntry> d_nzlist;   // photon lists of the resident split (k_nz_layout / k_nz_compact): per patch the pixels that hold a photon
    DevBuf<double> d_rate;      // per-pixel total rates of the photon split (strict boxes), B*H*W, on first use
    // the resident split's patch layout, grown together (cel_photon_split: grow_group); d_sbox is named last, so its capacity is the group's
    DevBuf<int4> d_sbox;
    DevBuf<int4> d_snz;         // nonzero rectangles of the resident sample patches (k_patch_nzbox)
    DevBuf<int64_t> d_soff;
    DevBuf<double> d_ssum;      // photons per (source, band) of the resident split, summed by the split kernel itself
    DevBuf<int> d_nnz, d_nzmode;   // ... and its photon lists' per-patch counts, modes and offsets
    DevBuf<int64_t> d_nzoff;
    DevBuf<double> d_stats;
    // device-resident slice sampler (cel_slice_locations): chain state, proposal set, per-round outputs
    DevBuf<char> d_slice;
    std::unique_ptr<cel_sources, SourcesDeleter> slice_prop;
    DevBuf<char> d_sgen;        // the general slice sampler's state (cel_slice_sample)
    std::unique_ptr<cel_sources, SourcesDeleter> sgen_prop;
    double last_entries = 0;
    bool counted = false;            // in ctx->live
    DevBuf<int> d_dirty;             // per tile: touched by a changed source's box (the incremental render)
    // the one-launch path of a small star field (k_small_stars.h): per-block partials + per-band arrival counters
    MappedBuf<double> h_small;
    double *d_small = nullptr;       // the device address of h_small (not owned)
    DevBuf<double> d_small_consts;
    unsigned long long small_seq = 0;
    bool llband_on_host = false;  // the last render's per-band sums were formed on the host (the small path): in h_llband
    double h_llband[MAX_BANDS] = {0};
    bool small_off = false;       // a part once held more stars than the kernel stages: the general path from then on
};

// (SourceStamps, field_state.h: gen, uid, full_gen, row_gen, n_gal, h_type and the three functions that write them)
struct cel_sources : SourceStamps {
    cel_ctx *ctx = nullptr;
    bool counted = false;          // in ctx->live
    int64_t cap = 0, S = 0;
    int B = 0;
    DevBuf<int> d_type;
    DevBuf<double> d_radec, d_counts, d_shape;
};

// The launch order of the tiles matters only when there are more tiles than the chip runs at once (2048 waves of the
// general kernel): below that every tile starts at once whatever the order, and a sort + its launch is all cost.
// A frame of few tiles is rendered by several one-wave blocks per tile (k_render_hw<, PARTS>, k_render_hw.h): 4 while even
// that many fit the chip's 2 048 wave slots at once (512 tiles), 2 up to 3 072 tiles (CEL_OPT_TILE_PARTS: 0 = this rule,
// 1 / 2 / 4 = always that many).  Measured on one rank's strip of the benchmark field cut 8 ways (1 280 tiles): one wave per
// tile 0.37 ms, two 0.21, four 0.25-0.29 -- every part pays its tile set-up and slab traffic, and 5 120 blocks are 2.5
// rounds of the chip.  (A tile whose list is short uses fewer of its parts: one per HW_PART_ENTRIES entries.)  The 32 x 64 layout's general kernel only; the star-tile kernels and the diagnostic instantiation
// keep one wave per tile.
static inline int tile_parts_of(const cel_ctx *c, const cel_images *im) {
    if (im->TW != 32 || c->variant == 0) return 1;
    if (c->tile_parts) return c->tile_parts;
    const int64_t T = (int64_t)im->B * im->ntx * im->nty;
    return T <= 512 ? 4 : (T <= 3072 ? 2 : 1);
}
static inline int tile_order_of(const cel_ctx *c, const cel_images *im) {
    return ((int64_t)im->B * im->ntx * im->nty * tile_parts_of(c, im) > 2048) ? c->tile_order : 0;
}

static bool prof_alloc(Prof &p) {
    if (p.ev) return true;
    p.ev = (hipEvent_t *)calloc(2 * Prof::PAIRS, sizeof(hipEvent_t));
    if (!p.ev) return false;
    for (int i = 0; i < 2 * Prof::PAIRS; i++)
        if (hipEventCreate(&p.ev[i]) != hipSuccess) return false;
    return true;
}
// read the oldest outstanding pair; `wait`: block until it has completed
static bool prof_harvest_one(Prof &p, bool wait) {
    if (p.count == 0) return false;
    const int t = (p.head - p.count + Prof::PAIRS) % Prof::PAIRS;
    if (wait) (void)hipEventSynchronize(p.ev[2 * t + 1]);
    else if (hipEventQuery(p.ev[2 * t + 1]) != hipSuccess) return false;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.ev[2 * t], p.ev[2 * t + 1]) == hipSuccess) {
        p.sum_ms[p.kid[t]] += ms;
        p.n[p.kid[t]] += 1;
    }
    p.count--;
    return true;
}
// reserve a pair for kernel k; returns the index of its first event, -1 when profiling is off
static int prof_slot(cel_ctx *c, int k) {
    if (!c->profile) return -1;
    // level 2: the small kernels around a render (prep, binning, reduction) go unbracketed -- an event pair costs the host
    // ~10 us per launch, 3 % of a 1.35 ms step when every kernel carries one
    if (c->profile >= 2 && (k == CEL_K_PREP || k == CEL_K_BIN || k == CEL_K_REDUCE)) return -1;
    // level 3: a SAMPLE of the evaluating launches -- every fourth of a kernel -- for steps so short that the pair's ~10 us
    // of host time is a fifth of what is being measured (configs[1]: a 44 us step)
    if (c->profile == 3 && (c->prof.seen[k]++ & 3) != 0) return -1;
    Prof &p = c->prof;
    if (!prof_alloc(p)) return -1;
    if (p.count == Prof::PAIRS) prof_harvest_one(p, true);
    else if (p.count > Prof::PAIRS / 2) { if (prof_harvest_one(p, false)) prof_harvest_one(p, false); }
    const int t = p.head;
    p.head = (p.head + 1) % Prof::PAIRS;
    p.count++;
    p.kid[t] = k;
    return 2 * t;
}
static int prof_begin(cel_ctx *c, int k) {
    const int i = prof_slot(c, k);
    if (i >= 0) (void)hipEventRecord(c->prof.ev[i], c->stream);
    return i;
}
static void prof_end(cel_ctx *c, int i) {
    if (i >= 0) (void)hipEventRecord(c->prof.ev[i + 1], c->stream);
}
// The step's own kernels (prep, binning, render, reduce) are timed WITHOUT marker packets: an event
// pair is reserved here and handed to hipExtLaunchKernelGGL, which stamps it from the dispatch's own
// start / completion signals.  A hipEventRecord between two kernels opens a ~10 us bubble in the
// queue (rocprofv3 kernel trace): four of them per 1.6 ms step were 2 % of what was being measured.
#define EV0(c, i) ((i) >= 0 ? (c)->prof.ev[(i)] : (hipEvent_t) nullptr)
#define EV1(c, i) ((i) >= 0 ? (c)->prof.ev[(i) + 1] : (hipEvent_t) nullptr)
// launch with optional start / stop events attached to the dispatch.  hipExtLaunchKernelGGL takes its arguments by their
// own types, so a buffer is handed over as its pointer (ext_arg)
template <class T> static inline T ext_arg(const T &v) { return v; }
template <class T, unsigned F> static inline T *ext_arg(const Buf<T, F> &b) { return b.get(); }
template <class K, class... A>
static inline void ext_launch(K kernel, dim3 grid, dim3 block, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const A &...a) {
    hipExtLaunchKernelGGL(kernel, grid, block, 0, st, e0, e1, 0, ext_arg(a)...);
}
#define LAUNCH_EV(kernel, grid, block, st, e0, e1, ...)                                              \
    do {                                                                                             \
        hipEvent_t e0_ = (e0), e1_ = (e1);                                                           \
        if (e0_ || e1_) ext_launch(kernel, grid, block, st, e0_, e1_, __VA_ARGS__);                  \
        else hipLaunchKernelGGL(kernel, grid, block, 0, st, __VA_ARGS__);                            \
    } while (0)
static void prof_collect(cel_ctx *c) {   // after a stream synchronise: everything outstanding has completed
    while (prof_harvest_one(c->prof, true)) {}
}

static double host_bounding_radius(const double *mu, const double *cov, int K, double error,
                                   const double *center) {
    double q = 1.0 - error;
    double rsq = -2.0 * log1p(-q);   // chi2.ppf(1 - error, 2)
    double best = -INFINITY;
    for (int i = 0; i < K; i++) {
        const double *c = cov + 4 * i;
        double s1 = sqrt(c[0]), s2 = sqrt(c[3]);
        double rho = c[1] / (s1 * s2);
        double A11 = s1, A21 = rho * s2, A22 = s2 * sqrt(1.0 - rho * rho);
        double An = 1.0 / rsq * (1.0 / (A11 * A11) + (A21 * A21) / (A22 * A22));
        double Bn = 1.0 / rsq * (-2.0 * A21 / (A11 * (A22 * A22)));
        double Cn = 1.0 / rsq * 1.0 / (A22 * A22);
        double maj = pow(0.5 * (An + Cn - sqrt(Bn * Bn + (An - Cn) * (An - Cn))), -0.5);
        double d0 = mu[2 * i] - (center ? center[0] : 0.0), d1 = mu[2 * i + 1] - (center ? center[1] : 0.0);
        double cand = maj + sqrt(d0 * d0 + d1 * d1);
        if (cand > best) best = cand;
    }
    return best;
}

static void band_to_dev(const cel_band &h, BandDev &d) {
    d.eps = h.eps;
    for (int k = 0; k < K_PSF; k++) {
        d.w[k] = h.w[k];
        d.mux[k] = h.mu[2 * k]; d.muy[k] = h.mu[2 * k + 1];
        d.cxx[k] = h.cov[4 * k]; d.cxy[k] = h.cov[4 * k + 1]; d.cyy[k] = h.cov[4 * k + 3];
    }
    for (int i = 0; i < 2; i++) { d.rho[i] = h.rho[i]; d.phi[i] = h.phi[i]; }
    for (int i = 0; i < 4; i++) { d.ups[i] = h.ups[i]; d.ups_inv[i] = h.ups_inv[i]; }
    d.R = h.R;
}

static int copy_in(void *dst, const void *src, size_t bytes, int mem, hipStream_t st) {
    if (bytes == 0) return CEL_OK;
    if (mem == CEL_DEVICE) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    } else {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));   // pageable source must stay valid
    }
    return CEL_OK;
}

static int copy_out(void *dst, const void *src, size_t bytes, int mem, hipStream_t st) {
    if (bytes == 0) return CEL_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, mem == CEL_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CEL_OK;
}

// One launch of k_patch_ll_hw<MODE, TZ>: a field per kernel parameter (k_patch_ll.h describes them) behind bands, B, H and W, which
// launch_patch_ll takes from the image set.  The defaults are the plain launch's: one block per job, in job order, one value per job.
template <typename TZ> struct PatchLlJob {
    int64_t P = 0;
    const SrcRec *recs = nullptr;
    const int *owner = nullptr;
    const int4 *pbox = nullptr;
    const int64_t *offsets = nullptr;
    const TZ *data = nullptr;
    const double *nelec = nullptr;
    const int4 *nzbox = nullptr;
    double Tdrop = 0.0, *out = nullptr;
    const int *job_order = nullptr;
    int nsplit = 1;
    const int *job_count = nullptr, *nzmode = nullptr;
    int encoded = 0, ostride = 0;
};
// the usual job: P proposals on the patches their owners name, against the observed image
template <typename TZ> static PatchLlJob<TZ> patch_ll_job(const cel_ctx *c, const cel_images *im, int64_t P, const int *owner, double *out,
                                                          const int4 *pbox, const int64_t *offsets, const TZ *data) {
    PatchLlJob<TZ> j;
    j.P = P; j.recs = im->d_recs; j.owner = owner; j.pbox = pbox; j.offsets = offsets; j.data = data; j.nelec = im->d_nelec;
    j.Tdrop = c->tail_T; j.out = out;
    return j;
}
// `pi`: a profile slot (prof_slot) whose event pair rides on the dispatch, or -1
template <int MODE, typename TZ>
static void launch_patch_ll(cel_ctx *c, const cel_images *im, const PatchLlJob<TZ> &j, int64_t blocks, hipStream_t st, int pi = -1) {
    LAUNCH_EV((k_patch_ll_hw<MODE, TZ>), dim3((unsigned)blocks), dim3(64), st, EV0(c, pi), EV1(c, pi), (const BandDev *)im->d_bands, im->B,
              j.P, j.recs, j.owner, j.pbox, j.offsets, j.data, j.nelec, im->H, im->W, j.nzbox, j.Tdrop, j.out, j.job_order, j.nsplit,
              j.job_count, j.nzmode, j.encoded, j.ostride);
}
// the stamp-mass form (MODE 3): P sources' unit stamps summed over their own boxes, a block per (source, band) job or entry of `jobs`
static void launch_stamp_mass(cel_ctx *c, const cel_images *im, int64_t P, const int *owner, double *out, int64_t blocks, const int *jobs = nullptr) {
    PatchLlJob<double> j;
    j.P = P; j.recs = im->d_recs; j.owner = owner; j.Tdrop = c->tail_T; j.out = out; j.job_order = jobs;
    launch_patch_ll<3>(c, im, j, blocks, c->stream);
}

extern "C" {

int cel_abi_version(void) { return CEL_ABI_VERSION; }
const char *cel_last_error(void) { return g_err; }

int cel_device_count(int *n) {
    if (!n) return fail(CEL_ERR_INVALID, "cel_device_count: null output");
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *n = c;
    return CEL_OK;
}

int cel_ctx_create(int device, void *stream, cel_ctx **out) {
    if (!out) return fail(CEL_ERR_INVALID, "cel_ctx_create: null output");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(CEL_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU fallback");
    if (device < 0 || device >= n) return fail(CEL_ERR_INVALID, "device %d out of range [0,%d)", device, n);
    HIP_TRY(hipSetDevice(device));
    cel_ctx *c = new (std::nothrow) cel_ctx();
    if (!c) return fail(CEL_ERR_NOMEM, "out of host memory");
    c->device = device;
    if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { delete c; return fail(CEL_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
        c->own_stream = true;
    }
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) c->n_cu = ncu;
    }
    hipError_t e = c->mail.grow(1, 1, c->stream);
    if (e != hipSuccess) { delete c; return fail(CEL_ERR_HIP, "pinned readback buffer: %s", hipGetErrorString(e)); }
    // profile constants, normalised as mixture_profiles.py:13,19
    double amp[K_PROF], var[K_PROF], se = 0.0, sd = 0.0;
    for (int i = 0; i < 6; i++) se += H_EXP_AMP[i];
    for (int i = 0; i < 8; i++) sd += H_DEV_AMP[i];
    for (int i = 0; i < 6; i++) { amp[i] = H_EXP_AMP[i] / se; var[i] = H_EXP_VAR[i]; }
    for (int i = 0; i < 8; i++) { amp[6 + i] = H_DEV_AMP[i] / sd; var[6 + i] = H_DEV_VAR[i]; }
    double ic[64], lc[64];
    log_tab_fill(ic, lc);
    if ((e = hipMemcpyToSymbol(HIP_SYMBOL(c_prof_amp), amp, sizeof(amp))) != hipSuccess ||
        (e = hipMemcpyToSymbol(HIP_SYMBOL(c_prof_var), var, sizeof(var))) != hipSuccess ||
        (e = hipMemcpyToSymbol(HIP_SYMBOL(c_log_ic), ic, sizeof(ic))) != hipSuccess ||
        (e = hipMemcpyToSymbol(HIP_SYMBOL(c_log_lc), lc, sizeof(lc))) != hipSuccess) {
        (void)cel_ctx_destroy(c);           // (the stream and the pinned block go with it)
        return fail(CEL_ERR_HIP, "hipMemcpyToSymbol: %s", hipGetErrorString(e));
    }
    *out = c;
    return CEL_OK;
}

int cel_ctx_destroy(cel_ctx *c) {
    if (!c) return CEL_OK;
    if (c->live > 0)        // their destructors synchronise this context's stream: destroy them first
        return fail(CEL_ERR_INVALID, "cel_ctx_destroy: %d image / source sets of this context are still alive", c->live);
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->prof.ev)
        for (int i = 0; i < 2 * Prof::PAIRS; i++)
            if (c->prof.ev[i]) (void)hipEventDestroy(c->prof.ev[i]);
    free(c->prof.ev);
    for (int k = 0; k < 2; k++) if (c->slice_ev[k]) (void)hipEventDestroy(c->slice_ev[k]);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return CEL_OK;
}

int cel_ctx_set_stream(cel_ctx *c, void *stream) {
    if (!c) return fail(CEL_ERR_INVALID, "null context");
    (void)hipStreamSynchronize(c->stream);
    if (c->own_stream) { (void)hipStreamDestroy(c->stream); c->own_stream = false; }
    if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    return CEL_OK;
}

int cel_ctx_synchronize(cel_ctx *c) {
    if (!c) return fail(CEL_ERR_INVALID, "null context");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CEL_OK;
}

int cel_ctx_set_option(cel_ctx *c, int key, double v) {
    if (!c) return fail(CEL_ERR_INVALID, "null context");
    switch (key) {
    case CEL_OPT_KERNEL:
        if (v != 0.0 && v != 1.0) return fail(CEL_ERR_INVALID, "CEL_OPT_KERNEL must be 0 or 1");
        c->variant = (int)v;
        return CEL_OK;
    case CEL_OPT_TAIL_LOG:
        if (v != v) { c->tail_T = 32.0; c->render_T = 24.0; return CEL_OK; }       // NaN: the defaults
        if (!(v >= 0.0) || v > 300.0) return fail(CEL_ERR_INVALID, "CEL_OPT_TAIL_LOG must be in [0, 300] (NaN: the defaults)");
        c->tail_T = v;
        c->render_T = v;
        return CEL_OK;
    case CEL_OPT_TAIL_LOG_SOURCE:
        if (v != v) { c->tail_T = 32.0; return CEL_OK; }
        if (!(v >= 0.0) || v > 300.0) return fail(CEL_ERR_INVALID, "CEL_OPT_TAIL_LOG_SOURCE must be in [0, 300] (NaN: the default)");
        c->tail_T = v;
        return CEL_OK;
    case CEL_OPT_INCREMENTAL:
        if (v != 0.0 && v != 1.0) return fail(CEL_ERR_INVALID, "CEL_OPT_INCREMENTAL must be 0 or 1");
        c->incremental = (int)v;
        return CEL_OK;
    case CEL_OPT_SPLIT_FULL_BOX:
        if (v != 0.0 && v != 1.0) return fail(CEL_ERR_INVALID, "CEL_OPT_SPLIT_FULL_BOX must be 0 or 1");
        c->split_full = (int)v;
        return CEL_OK;
    case CEL_OPT_SLICE_FUSE:
        if (!(v >= 0.0 && v <= 1e9) || v != floor(v)) return fail(CEL_ERR_INVALID, "CEL_OPT_SLICE_FUSE must be 0, 1 or a block count");
        c->slice_fuse = (int)v;
        return CEL_OK;
    case CEL_OPT_HONOUR_MASK:
        if (v != 0.0 && v != 1.0) return fail(CEL_ERR_INVALID, "CEL_OPT_HONOUR_MASK must be 0 or 1");
        c->honour_mask = (int)v;
        return CEL_OK;
    case CEL_OPT_SLICE_CONDITIONAL:
        static_assert(CEL_OPT_SLICE_CONDITIONAL == 18, "the key is 18 in every binding");
        if (v != 0.0 && v != 1.0) return fail(CEL_ERR_INVALID, "CEL_OPT_SLICE_CONDITIONAL must be 0 (the reference's conditional) or 1 (the exact one)");
        c->slice_conditional = (int)v;
        return CEL_OK;
    case CEL_OPT_GRAD_CONDITIONAL:
        static_assert(CEL_OPT_GRAD_CONDITIONAL == 19, "the key is 19 in every binding");
        if (v != 0.0 && v != 1.0) return fail(CEL_ERR_INVALID, "CEL_OPT_GRAD_CONDITIONAL must be 0 (the reference's conditional) or 1 (the exact one)");
        c->grad_conditional = (int)v;
        return CEL_OK;
    case CEL_OPT_COMP_CACHE:
        static_assert(CEL_OPT_COMP_CACHE == 20, "the key is 20 in every binding");
        if (v != 0.0 && v != 1.0) return fail(CEL_ERR_INVALID, "CEL_OPT_COMP_CACHE must be 0 or 1");
        c->comp_cache = (int)v;
        return CEL_OK;
    case CEL_OPT_SAMPLER_MASK:
        static_assert(CEL_OPT_SAMPLER_MASK == 21, "the key is 21 in every binding");
        if (v != 0.0 && v != 1.0) return fail(CEL_ERR_INVALID, "CEL_OPT_SAMPLER_MASK must be 0 (the samplers refuse a masked set) or 1 (the exact ones honour it)");
        c->sampler_mask = (int)v;
        return CEL_OK;
    case CEL_OPT_TILE_PARTS:
        if (v != 0.0 && v != 1.0 && v != 2.0 && v != 4.0) return fail(CEL_ERR_INVALID, "CEL_OPT_TILE_PARTS must be 0 (by the frame's size), 1, 2 or 4");
        c->tile_parts = (int)v;
        return CEL_OK;
    case CEL_OPT_PROFILE:
        if (v != 0.0 && v != 1.0 && v != 2.0 && v != 3.0) return fail(CEL_ERR_INVALID, "CEL_OPT_PROFILE must be 0, 1, 2 or 3");
        if (v != 0.0 && !prof_alloc(c->prof)) return fail(CEL_ERR_HIP, "CEL_OPT_PROFILE: cannot create the timing events");
        c->profile = (int)v;
        return CEL_OK;
    case CEL_OPT_TILE_ORDER:
        if (v != 0.0 && v != 1.0 && v != 2.0) return fail(CEL_ERR_INVALID, "CEL_OPT_TILE_ORDER must be 0, 1 or 2");
        c->tile_order = (int)v;
        return CEL_OK;
    case CEL_OPT_TILE_ROWS:
        if (v != 32.0 && v != 64.0) return fail(CEL_ERR_INVALID, "CEL_OPT_TILE_ROWS must be 32 or 64");
        c->tile_rows = (int)v;
        return CEL_OK;
    case CEL_OPT_TILE_TIMING:
        c->tile_timing = (v != 0.0);
        return CEL_OK;
    case CEL_OPT_TILE_LAYOUT:
        if (v != 0.0 && v != 1.0 && v != 2.0) return fail(CEL_ERR_INVALID, "CEL_OPT_TILE_LAYOUT must be 0, 1 or 2");
        c->tile_layout = (int)v;
        return CEL_OK;
    case CEL_OPT_PHOTON_LISTS:
        if (v != 0.0 && v != 1.0 && v != 2.0 && v != 4.0 && v != 5.0)
            return fail(CEL_ERR_INVALID, "CEL_OPT_PHOTON_LISTS must be 0, 1 or 2, or 4 or 5 (0 / 1 and the resident gradient at the photons)");
        c->nz_force = (int)v & 3;
        c->grad_nz = v >= 4.0;
        return CEL_OK;
    case CEL_OPT_SPLIT_REUSE:
        if (v != 0.0 && v != 1.0 && v != 2.0) return fail(CEL_ERR_INVALID, "CEL_OPT_SPLIT_REUSE must be 0, 1 or 2");
        c->split_reuse = (int)v;
        return CEL_OK;
    case CEL_OPT_STAR_TILES:
        if (v != 0.0 && v != 1.0 && v != 2.0 && v != 3.0) return fail(CEL_ERR_INVALID, "CEL_OPT_STAR_TILES must be 0, 1, 2 or 3");
        c->star_tiles = (int)v;
        return CEL_OK;
    case CEL_OPT_DEBUG:
        if (!(v >= 0.0) || v > 4095.0) return fail(CEL_ERR_INVALID, "CEL_OPT_DEBUG must be in [0, 4095]");
#ifndef CEL_ABLATE
        // the shipped library carries no ablation path: only the two result-preserving diagnostic bits exist
        if (((int)v) & ~(64 | 128))
            return fail(CEL_ERR_INVALID, "CEL_OPT_DEBUG: the timing-only ablation bits exist only in a -DCEL_ABLATE build "
                                         "(make -C desi-mcmc_amd/csrc ablate); this library accepts 64 and 128");
#endif
        c->debug = (int)v;
        return CEL_OK;
    }
    return fail(CEL_ERR_INVALID, "unknown option %d", key);
}

int cel_ctx_get_option(cel_ctx *c, int key, double *v) {
    if (!c || !v) return fail(CEL_ERR_INVALID, "null argument");
    switch (key) {
    case CEL_OPT_KERNEL: *v = c->variant; return CEL_OK;
    case CEL_OPT_TAIL_LOG: *v = c->render_T; return CEL_OK;
    case CEL_OPT_TAIL_LOG_SOURCE: *v = c->tail_T; return CEL_OK;
    case CEL_OPT_TILE_PARTS: *v = c->tile_parts; return CEL_OK;
    case CEL_OPT_INCREMENTAL: *v = c->incremental; return CEL_OK;
    case CEL_OPT_SPLIT_FULL_BOX: *v = c->split_full; return CEL_OK;
    case CEL_OPT_SLICE_FUSE: *v = c->slice_fuse; return CEL_OK;
    case CEL_OPT_HONOUR_MASK: *v = c->honour_mask; return CEL_OK;
    case CEL_OPT_SLICE_CONDITIONAL: *v = c->slice_conditional; return CEL_OK;
    case CEL_OPT_GRAD_CONDITIONAL: *v = c->grad_conditional; return CEL_OK;
    case CEL_OPT_COMP_CACHE: *v = c->comp_cache; return CEL_OK;
    case CEL_OPT_SAMPLER_MASK: *v = c->sampler_mask; return CEL_OK;
    case CEL_OPT_PROFILE: *v = (double)c->profile; return CEL_OK;
    case CEL_OPT_TILE_ORDER: *v = (double)c->tile_order; return CEL_OK;
    case CEL_OPT_TILE_ROWS: *v = c->tile_rows; return CEL_OK;
    case CEL_OPT_TILE_TIMING: *v = c->tile_timing ? 1.0 : 0.0; return CEL_OK;
    case CEL_OPT_TILE_LAYOUT: *v = c->tile_layout; return CEL_OK;
    case CEL_OPT_PHOTON_LISTS: *v = c->nz_force + (c->grad_nz ? 4 : 0); return CEL_OK;
    case CEL_OPT_STAR_TILES: *v = c->star_tiles; return CEL_OK;
    case CEL_OPT_SPLIT_REUSE: *v = c->split_reuse; return CEL_OK;
    case CEL_OPT_DEBUG: *v = c->debug; return CEL_OK;
    }
    return fail(CEL_ERR_INVALID, "unknown option %d", key);
}

// ---- images ---------------------------------------------------------------------------------
int cel_images_destroy(cel_images *im) {
    if (!im) return CEL_OK;
    (void)hipSetDevice(im->ctx->device);
    (void)hipStreamSynchronize(im->ctx->stream);
    if (im->ev_step) (void)hipEventDestroy(im->ev_step);
    if (im->counted) im->ctx->live--;
    delete im;                            // (the buffers and the proposal sets free themselves)
    return CEL_OK;
}

int cel_images_create(cel_ctx *c, int B, int H, int W, const cel_band *bands, cel_images **out) {
    if (!c || !bands || !out) return fail(CEL_ERR_INVALID, "cel_images_create: null argument");
    if (B < 1 || B > MAX_BANDS) return fail(CEL_ERR_INVALID, "B=%d out of range [1,%d]", B, MAX_BANDS);
    if (H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 34) return fail(CEL_ERR_INVALID, "bad image size %dx%d", H, W);
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<cel_images> im(new (std::nothrow) cel_images());   // (a failed creation frees what it allocated)
    if (!im) return fail(CEL_ERR_NOMEM, "out of host memory");
    im->ctx = c; im->B = B; im->H = H; im->W = W;
    im->full_H = H; im->win_y0 = 0;
    if (c->tile_layout == 1) { im->TW = HW_TW; im->TH = HW_TH; }
    else if (c->tile_layout == 2) { im->TW = QW_TW; im->TH = QW_TH; }
    else { im->TW = TILE_W; im->TH = c->tile_rows; }
    im->ntx = (W + im->TW - 1) / im->TW;
    im->nty = (H + im->TH - 1) / im->TH;
    im->nsx = (W + SUPER_W - 1) / SUPER_W;
    im->nsy = (H + SUPER_H - 1) / SUPER_H;
    BandDev hb[MAX_BANDS];
    for (int b = 0; b < B; b++) {
        im->hb[b] = bands[b];
        for (int k = 0; k < K_PSF; k++) {
            const double *cv = bands[b].cov + 4 * k;
            double det = cv[0] * cv[3] - cv[1] * cv[2];
            if (!(cv[0] > 0) || !(cv[3] > 0) || !(det > 0))
                return fail(CEL_ERR_INVALID, "band %d: PSF component %d covariance is not positive definite", b, k);
        }
        if (!(im->hb[b].R > 0.0))
            im->hb[b].R = host_bounding_radius(bands[b].mu, bands[b].cov, K_PSF, 0.001, nullptr);
        band_to_dev(im->hb[b], hb[b]);
    }
    im->star_one_segment = true;
    for (int b = 0; b < B; b++)
        for (int k = 0; k < K_PSF; k++) {      // star_setup's test (k_render_hw.h), on the host
            const BandDev &d = hb[b];
            const double inv = 1.0 / (d.cxx[k] * d.cyy[k] - d.cxy[k] * d.cxy[k]);
            const double rb_ = d.R + 2.0;
            const double emax = 0.5 * quad_max_rect_hw(d.cyy[k] * inv, -d.cxy[k] * inv, d.cxx[k] * inv, -rb_ - d.mux[k], rb_ - d.mux[k],
                                                       -rb_ - d.muy[k], rb_ - d.muy[k]);
            if (!(emax <= 0.999 * STAR_EMAX)) im->star_one_segment = false;
        }
    const int64_t npix = (int64_t)B * H * W;
    const int T = B * im->ntx * im->nty, NS = B * im->nsx * im->nsy;
    hipStream_t st = c->stream;
    HIP_TRY(im->d_bands.grow(B, B, st));
    HIP_TRY(hipMemcpy(im->d_bands, hb, sizeof(BandDev) * B, hipMemcpyHostToDevice));
    HIP_TRY(im->d_nelec.grow(npix, npix, st));
    HIP_TRY(im->d_lambda.grow(npix, npix, st));
    HIP_TRY(im->d_partials.grow(T, T, st));
    // per-band sums and the binning cursors (4 x u64) share one buffer: they ride back to the host in one copy; the
    // binning pass's saved cursors and its changed-at word lie behind them
    HIP_TRY(im->d_llband.grow(MAX_BANDS + BIN_WORDS, MAX_BANDS + BIN_WORDS, st));
    im->d_cursor = reinterpret_cast<unsigned long long *>(im->d_llband + MAX_BANDS);
    HIP_TRY(hipMemsetAsync(im->d_cursor, 0, sizeof(unsigned long long) * BIN_WORDS, st));
    HIP_TRY(im->d_tile_cnt.grow(T, T, st));
    HIP_TRY(im->d_tile_nstar.grow(T, T, st));
    HIP_TRY(im->d_tile_work.grow(T, T, st));
    HIP_TRY(im->d_tile_cost.grow(T, T, st));
    HIP_TRY(im->d_order.grow(T, T, st));
    HIP_TRY(im->d_tile_off.grow(T, T, st));
    HIP_TRY(im->d_sup_cnt.grow(NS, NS, st));
    HIP_TRY(im->d_sup_off.grow(NS, NS, st));
    HIP_TRY(im->d_stats.grow(2, 2, st));
    HIP_TRY(hipMemsetAsync(im->d_lambda, 0, sizeof(double) * npix, st));
    im->counted = true;
    c->live++;
    *out = im.release();
    return CEL_OK;
}

int cel_images_set_nelec(cel_images *im, const double *nelec, int mem) {
    if (!im || !nelec) return fail(CEL_ERR_INVALID, "cel_images_set_nelec: null argument");
    HIP_TRY(hipSetDevice(im->ctx->device));
    int rc = copy_in(im->d_nelec, nelec, sizeof(double) * (size_t)im->B * im->H * im->W, mem, im->ctx->stream);
    if (rc != CEL_OK) return rc;
    im->have_nelec = true;
    // new pixels drop the resident photon split (cel_samples_info reports S = 0, and every call that needs the split refuses
    // until the next resident cel_photon_split) with the stamp sums that split left for cel_stamp_mass
    im->new_pixels();
    // the image's range: 0 ... 65 535 everywhere lets the photon split keep its photons-left plane in 16 bits (k_split.h)
    // ... and the NaN counts per band: the mask (a block's count stays below 2^53: exact in a double)
    im->any_masked = false;
    {
        const int nbb = std::max(1, 512 / im->B), NB = nbb * im->B;     // blocks per band
        DevBuf<double> d_rng;
        HIP_TRY(d_rng.grow(3 * NB, 3 * NB, im->ctx->stream));
        hipLaunchKernelGGL(k_nelec_range, dim3(NB), dim3(256), 0, im->ctx->stream, (const double *)im->d_nelec,
                           (int64_t)im->H * im->W, nbb, d_rng);
        std::vector<double> h((size_t)3 * NB);
        HIP_TRY(hipMemcpyAsync(h.data(), d_rng, sizeof(double) * 3 * NB, hipMemcpyDeviceToHost, im->ctx->stream));
        HIP_TRY(hipStreamSynchronize(im->ctx->stream));
        double lo = INFINITY, hi = -INFINITY;
        int64_t bad = 0;
        for (int b = 0; b < im->B; b++) {
            im->masked[b] = 0;
            for (int k = b * nbb; k < (b + 1) * nbb; k++) {
                lo = fmin(lo, h[3 * k]); hi = fmax(hi, h[3 * k + 1]);
                im->masked[b] += (int64_t)h[3 * k + 2];
            }
            bad += im->masked[b];
        }
        im->any_masked = bad != 0;
        im->pixel_range((bad == 0) && (lo >= 0.0) && (hi <= 65535.0));
    }
    return CEL_OK;
}

int cel_images_mask_info(cel_images *im, int64_t *masked) {
    if (!im || !masked) return fail(CEL_ERR_INVALID, "cel_images_mask_info: null argument");
    for (int b = 0; b < im->B; b++) masked[b] = im->masked[b];
    return CEL_OK;
}

// the entry points that have not been taught about a mask refuse a masked set, before they launch anything
static int refuse_masked(const cel_images *im, const char *who) {
    if (!im->any_masked) return CEL_OK;
    int64_t n = 0;
    for (int b = 0; b < im->B; b++) n += im->masked[b];
    return fail(CEL_ERR_INVALID, "%s: the image set holds %lld masked pixels (NaN counts, cel_images_set_nelec) and this call does not honour a mask",
                who, (long long)n);
}

// ... and the calls of the Gibbs sweep that have been taught (photon split, stamp masses, flux step) do so unless the context asks
// for the mask to be honoured (CEL_OPT_HONOUR_MASK); honours_mask: this call takes its masked path
static inline bool honours_mask(const cel_images *im) { return im->any_masked && im->ctx->honour_mask != 0; }
static int refuse_masked_unless_honoured(const cel_images *im, const char *who) {
    return im->ctx->honour_mask ? CEL_OK : refuse_masked(im, who);
}
// ... and the device samplers of the EXACT conditional and the exact resident gradient once CEL_OPT_SAMPLER_MASK says so as well:
// samplers_honour_mask: this call charges the OBSERVED mass (k_stamp_mass_masked) and its derivative (k_mass_grad_masked), one for
// one in place of the plain kernels.  The reference's conditional charges the sum of the PSF weights, which is wrong beside a mask:
// a call that does not run the exact conditional keeps being refused.
static inline bool samplers_honour_mask(const cel_images *im) { return honours_mask(im) && im->ctx->sampler_mask != 0; }
static int refuse_masked_sampler(const cel_images *im, const char *who, bool exact_call) {
    return (exact_call && im->ctx->honour_mask && im->ctx->sampler_mask) ? CEL_OK : refuse_masked(im, who);
}
// the exact conditional's mass launch for the P slots of a proposal set (the records WITH boxes are on the device): launch_stamp_mass,
// or its observed twin on the same blocks, job list and owners -- one launch either way
static void launch_proposal_mass(cel_ctx *c, const cel_images *im, int64_t P, const int *owner, double *out, int64_t blocks, const int *jobs = nullptr) {
    if (samplers_honour_mask(im))
        hipLaunchKernelGGL(k_stamp_mass_masked, dim3((unsigned)blocks), dim3(64), 0, c->stream, im->d_bands, im->B, im->H, im->W, P,
                           im->d_recs, (const double *)im->d_nelec, c->tail_T, out, jobs, owner);
    else
        launch_stamp_mass(c, im, P, owner, out, blocks, jobs);
}
// ... and the launch of that mass's derivative sums (k_mass_grad.h), P * B * PGRAD_PARTS blocks
static void launch_mass_grad(cel_ctx *c, const cel_images *im, int64_t P, const int *owner, double *sums) {
    const dim3 grid((unsigned)(P * im->B * PGRAD_PARTS));
    if (samplers_honour_mask(im))
        hipLaunchKernelGGL(k_mass_grad_masked, grid, dim3(64), 0, c->stream, im->d_bands, im->B, P, im->d_recs, owner,
                           (const double *)im->d_nelec, im->H, im->W, sums);
    else
        hipLaunchKernelGGL(k_mass_grad, grid, dim3(64), 0, c->stream, im->d_bands, im->B, P, im->d_recs, owner, sums);
}

int cel_images_set_epsilon(cel_images *im, int band, double eps) {
    if (!im || band < 0 || band >= im->B) return fail(CEL_ERR_INVALID, "cel_images_set_epsilon: bad band");
    HIP_TRY(hipSetDevice(im->ctx->device));
    im->hb[band].eps = eps;
    im->new_sky_level();
    // stream-ordered, no host synchronisation (Gibbs calls this per band per sweep)
    hipLaunchKernelGGL(k_set_eps, dim3(1), dim3(1), 0, im->ctx->stream, im->d_bands, band, eps);
    HIP_TRY(hipGetLastError());
    return CEL_OK;
}

int cel_images_set_window(cel_images *im, int y0, int full_H) {
    if (!im) return fail(CEL_ERR_INVALID, "null images");
    if (y0 < 0 || full_H < 1 || (int64_t)y0 + im->H > full_H)
        return fail(CEL_ERR_INVALID, "window rows [%d, %d) do not fit a %d-row frame", y0, y0 + im->H, full_H);
    if (y0 == im->win_y0 && full_H == im->full_H) return CEL_OK;       // the window it has: nothing is cut anew, nothing dropped
    im->win_y0 = y0;
    im->full_H = full_H;
    im->new_window();
    return CEL_OK;
}

int cel_images_set_noise_rows(cel_images *im, int y0, int y1) {
    if (!im) return fail(CEL_ERR_INVALID, "null images");
    if (y0 < 0 || y1 < y0) return fail(CEL_ERR_INVALID, "cel_images_set_noise_rows: rows [%d, %d)", y0, y1);
    im->noise_y0 = y0;
    im->noise_y1 = y1;
    return CEL_OK;
}

int cel_images_get_band(cel_images *im, int band, cel_band *out) {
    if (!im || !out || band < 0 || band >= im->B) return fail(CEL_ERR_INVALID, "cel_images_get_band: bad argument");
    *out = im->hb[band];
    return CEL_OK;
}

int cel_images_get_lambda(cel_images *im, double *out, int mem) {
    if (!im || !out) return fail(CEL_ERR_INVALID, "cel_images_get_lambda: null argument");
    HIP_TRY(hipSetDevice(im->ctx->device));
    return copy_out(out, im->d_lambda, sizeof(double) * (size_t)im->B * im->H * im->W, mem, im->ctx->stream);
}

int cel_images_device_ptrs(cel_images *im, void **nelec, void **lambda) {
    if (!im) return fail(CEL_ERR_INVALID, "null images");
    if (nelec) {        // the caller may write it, at any time: no assumption about its range any more, no Poisson partials kept
        *nelec = im->d_nelec; im->pixels_handed_out();
    }
    if (lambda) *lambda = im->d_lambda;
    return CEL_OK;
}

int cel_images_loglik_device(cel_images *im, void **ll_band) {
    if (!im || !ll_band) return fail(CEL_ERR_INVALID, "cel_images_loglik_device: null argument");
    if (im->llband_on_host) {
        // the one-launch path of a small star field adds its blocks' partials on the host: put the sums where every other
        // render leaves them
        cel_ctx *c = im->ctx;
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipMemcpyAsync(im->d_llband, im->h_llband, sizeof(double) * im->B, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        im->llband_on_host = false;
    }
    *ll_band = im->d_llband;
    return CEL_OK;
}

// ---- sources --------------------------------------------------------------------------------
int cel_sources_destroy(cel_sources *s) {
    if (!s) return CEL_OK;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    if (s->counted) s->ctx->live--;
    delete s;
    return CEL_OK;
}

int cel_sources_create(cel_ctx *c, int64_t capacity, int B, cel_sources **out) {
    if (!c || !out) return fail(CEL_ERR_INVALID, "cel_sources_create: null argument");
    if (capacity < 1 || capacity > ((int64_t)1 << 30)) return fail(CEL_ERR_INVALID, "bad capacity");
    if (B < 1 || B > MAX_BANDS) return fail(CEL_ERR_INVALID, "B=%d out of range", B);
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<cel_sources> s(new (std::nothrow) cel_sources());   // (a failed creation frees what it allocated)
    if (!s) return fail(CEL_ERR_NOMEM, "out of host memory");
    s->ctx = c; s->cap = capacity; s->B = B;
    s->created();
    HIP_TRY(s->d_type.grow(capacity, capacity, c->stream));
    HIP_TRY(s->d_radec.grow(2 * capacity, 2 * capacity, c->stream));
    HIP_TRY(s->d_counts.grow(B * capacity, B * capacity, c->stream));
    HIP_TRY(s->d_shape.grow(4 * capacity, 4 * capacity, c->stream));
    s->counted = true;
    s->ctx->live++;
    *out = s.release();
    return CEL_OK;
}

int cel_sources_set(cel_sources *s, int64_t S, const int32_t *type, const double *radec,
                    const double *counts, const double *shape, int mem) {
    if (!s || !type || !radec || !counts || !shape) return fail(CEL_ERR_INVALID, "cel_sources_set: null argument");
    if (S < 0 || S > s->cap) return fail(CEL_ERR_INVALID, "S=%lld exceeds capacity %lld", (long long)S, (long long)s->cap);
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    if (S > 0) {
        const hipMemcpyKind kind = (mem == CEL_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        HIP_TRY(hipMemcpyAsync(s->d_type, type, sizeof(int) * S, kind, st));
        HIP_TRY(hipMemcpyAsync(s->d_radec, radec, sizeof(double) * 2 * S, kind, st));
        HIP_TRY(hipMemcpyAsync(s->d_counts, counts, sizeof(double) * s->B * S, kind, st));
        HIP_TRY(hipMemcpyAsync(s->d_shape, shape, sizeof(double) * 4 * S, kind, st));
        if (mem != CEL_DEVICE) HIP_TRY(hipStreamSynchronize(st));   // pageable sources must stay valid: one sync for the four
    }
    s->S = S;
    s->all_rows_changed(true);
    if (mem != CEL_DEVICE) s->types_known(type, S);
    return CEL_OK;
}

// the catalogue as the device holds it, copied to host arrays (any may be NULL): the device samplers rewrite it in place
// (cel_flux_conditionals the counts, the slice samplers the locations and shapes), and this is how a caller or a test sees what
// they left
int cel_sources_get(cel_sources *s, int32_t *type, double *radec, double *counts, double *shape) {
    if (!s) return fail(CEL_ERR_INVALID, "cel_sources_get: null argument");
    HIP_TRY(hipSetDevice(s->ctx->device));
    hipStream_t st = s->ctx->stream;
    const int64_t S = s->S;
    if (S > 0) {
        if (type) HIP_TRY(hipMemcpyAsync(type, s->d_type, sizeof(int) * S, hipMemcpyDeviceToHost, st));
        if (radec) HIP_TRY(hipMemcpyAsync(radec, s->d_radec, sizeof(double) * 2 * S, hipMemcpyDeviceToHost, st));
        if (counts) HIP_TRY(hipMemcpyAsync(counts, s->d_counts, sizeof(double) * s->B * S, hipMemcpyDeviceToHost, st));
        if (shape) HIP_TRY(hipMemcpyAsync(shape, s->d_shape, sizeof(double) * 4 * S, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return CEL_OK;
}

// n rows of the catalogue replaced (host arrays, packed: idx[n], type[n], radec[n][2], counts[n][B], shape[n][4]): what a
// caller that changed ONE source between two evaluations uploads instead of the whole catalogue (the RJ moves and slice
// steps of CelestePy/util/infer/mcmc_transitions.py:37-152 call celeste_likelihood after every such change)
int cel_sources_set_rows(cel_sources *s, int64_t n, const int32_t *idx, const int32_t *type, const double *radec,
                         const double *counts, const double *shape) {
    if (!s || n < 0 || (n > 0 && (!idx || !type || !radec || !counts || !shape)))
        return fail(CEL_ERR_INVALID, "cel_sources_set_rows: null argument");
    for (int64_t i = 0; i < n; i++)
        if (idx[i] < 0 || idx[i] >= s->S) return fail(CEL_ERR_INVALID, "cel_sources_set_rows: row %d outside the catalogue's %lld", idx[i], (long long)s->S);
    if (n == 0) return CEL_OK;
    {   // a row named twice would be written by two threads of k_scatter_rows at once: the last writer is undefined
        std::vector<int32_t> seen(idx, idx + n);
        std::sort(seen.begin(), seen.end());
        for (int64_t i = 1; i < n; i++)
            if (seen[i] == seen[i - 1]) return fail(CEL_ERR_INVALID, "cel_sources_set_rows: row %d is named twice", seen[i]);
    }
    cel_ctx *c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int B = s->B;
    // one staging buffer: idx, type (ints), then radec, counts, shape (doubles)
    const size_t ints = ((size_t)(2 * n) * sizeof(int) + 7) & ~(size_t)7;
    const size_t bytes = ints + sizeof(double) * (size_t)n * (2 + B + 4);
    char *d = nullptr;
    int rc = scratch_get(c, SCR_HOST_IO, bytes, (void **)&d);
    if (rc) return rc;
    std::vector<char> h(bytes);
    memcpy(h.data(), idx, sizeof(int) * n);
    memcpy(h.data() + sizeof(int) * n, type, sizeof(int) * n);
    double *hd = reinterpret_cast<double *>(h.data() + ints);
    memcpy(hd, radec, sizeof(double) * 2 * n);
    memcpy(hd + 2 * n, counts, sizeof(double) * B * n);
    memcpy(hd + (2 + B) * n, shape, sizeof(double) * 4 * n);
    HIP_TRY(hipMemcpyAsync(d, h.data(), bytes, hipMemcpyHostToDevice, st));
    const double *dd = reinterpret_cast<const double *>(d + ints);
    hipLaunchKernelGGL(k_scatter_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, B, (const int *)d, (const int *)d + n,
                       dd, dd + 2 * n, dd + (2 + B) * n, s->d_type, s->d_radec, s->d_counts, s->d_shape);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));          // the pageable staging vector goes out of scope
    s->rows_replaced(s->S, n, idx, type);        // (the row stamps: render_impl's incremental path)
    return CEL_OK;
}

// ---- prep + bin (shared by field and stamps) ------------------------------------------------
static int ensure_recs(cel_images *im, int64_t n) {
    if (n <= im->d_recs.cap) return CEL_OK;
    im->records_regrown();
    const int64_t cap = n + n / 4 + 64;
    HIP_TRY(grow_group(im->ctx->stream, im->d_boxes, cap, im->d_kind, cap, im->d_status, cap, im->d_recs, cap));
    return CEL_OK;
}

static double rsq_galaxy() {
    double q = 1.0 - 1e-5;           // celeste_galaxy_conditionals.py:207 error=1e-5
    return -2.0 * log1p(-q);         // scipy.stats.chi2.ppf(q, 2)
}

// step != 0 (a render whose binning may be skipped, never with d_live or nobox): k_prep compares every (box, kind) with what
// stands in the tables before it stores (k_prep_bin.h)
static int run_prep(cel_images *im, cel_sources *src, const int *d_live = nullptr, int nobox = 0, unsigned long long step = 0) {
    cel_ctx *c = im->ctx;
    int64_t n = src->S * im->B;
    int rc = ensure_recs(im, n > 0 ? n : 1);
    if (rc) return rc;
    if (n == 0) { im->records_written(src->gen, 0); return CEL_OK; }
    int pi = prof_slot(c, CEL_K_PREP);
    LAUNCH_EV(k_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), c->stream, EV0(c, pi), EV1(c, pi), im->d_bands, im->B,
              im->full_H, im->W, im->win_y0, im->H, src->S, src->d_type, src->d_radec, src->d_counts, src->d_shape,
              rsq_galaxy(), im->d_recs, im->d_boxes, im->d_kind, im->d_status, im->d_cursor, (d_live || nobox) ? 0ull : step, d_live, nobox);
    HIP_TRY(hipGetLastError());
    im->records_written((d_live || nobox) ? 0 : src->gen, src->S);      // a partial table is nobody else's
    return CEL_OK;
}

// host copies of the boxes and status of every (band, source) of `src` (20 B each, not the 128-B
// records); reused until the sources or the window change
static int host_boxes(cel_images *im, cel_sources *src) {
    if (im->rec.host_boxes_of(*src)) return CEL_OK;
    int rc = im->rec.of(*src) ? CEL_OK : run_prep(im, src);
    if (rc) return rc;
    const int64_t n = src->S * im->B;
    im->h_boxes.resize((size_t)n);
    im->h_status.resize((size_t)n);
    if (n) {
        hipStream_t st = im->ctx->stream;
        HIP_TRY(hipMemcpyAsync(im->h_boxes.data(), im->d_boxes, sizeof(int4) * n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(im->h_status.data(), im->d_status, sizeof(int) * n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    im->host_boxes_read(src->gen);
    return CEL_OK;
}

// internal render flag: sources take part only strictly inside their boxes on the low side
// (x > x0, y > y0), the photon split's membership rule (celeste_sample_sources.pyx:50-51)
#define CEL_RENDER_STRICT 4
// internal render flag: the caller reads the tile lists afterwards (the E-step's tile walk): the general path
#define CEL_RENDER_KEEP_LISTS 16
static int render_impl(cel_images *im, cel_sources *src, int flags, double *ll_band, double *ll_total, double *lambda_out);

int cel_render_field(cel_images *im, cel_sources *src, int flags, double *ll_band, double *ll_total) {
    if (flags & ~(CEL_RENDER_LOGLIK | CEL_RENDER_NO_STORE)) return fail(CEL_ERR_INVALID, "cel_render_field: unknown flag bits");
    return render_impl(im, src, flags, ll_band, ll_total, nullptr);
}

// A small star field in one launch (k_small_stars.h): prep, binning, render and the per-band reduction.  *done = false when a
// part of a tile held more stars than the kernel stages (the caller then takes the general path, from now on).
static int render_small_stars(cel_images *im, cel_sources *src, int flags, bool *done) {
    cel_ctx *c = im->ctx;
    hipStream_t st = c->stream;
    const int64_t S = src->S;
    const int B = im->B;
    *done = false;
    int rc = ensure_recs(im, S * B);
    if (rc) return rc;
    const int nblk = B * im->ntx * im->nty * SMALL_NB, nblk_band = im->ntx * im->nty * SMALL_NB;
    if (!im->h_small) {
        // the blocks' partials and the overflow word behind them live in pinned, device-mapped, coherent HOST memory: the
        // kernel stores them over PCIe itself (5 KB at configs[1]) and the step needs no copy command behind the kernel
        // -- a D2H copy of this size cost the step ~8 us of queue latency
        HIP_TRY(im->h_small.grow(nblk + 1, nblk + 1, st));
        memset(im->h_small, 0, sizeof(double) * (nblk + 1));
        HIP_TRY(hipHostGetDevicePointer((void **)&im->d_small, im->h_small, 0));
        // the bands' star-pass constants, once (the PSF and the WCS of an image set do not change)
        HIP_TRY(im->d_small_consts.grow(SMALL_CONSTS * B, SMALL_CONSTS * B, st));
        hipLaunchKernelGGL(k_small_consts, dim3(B), dim3(64), 0, st, (const BandDev *)im->d_bands, im->d_small_consts);
    }
    RenderArgs a;
    memset(&a, 0, sizeof(a));
    a.bands = im->d_bands; a.recs = im->d_recs; a.nelec = im->d_nelec; a.lambda = im->d_lambda; a.partials = im->d_small;
    a.S = S; a.B = B; a.H = im->H; a.W = im->W; a.ntx = im->ntx; a.nty = im->nty;
    a.flags = flags; a.variant = c->variant; a.tail_T = c->render_T;
    SmallArgs x;
    x.radec = src->d_radec; x.counts = src->d_counts;
    x.recs = im->d_recs; x.boxes = im->d_boxes; x.kind = im->d_kind; x.status = im->d_status;
    x.partials = im->d_small;
    x.flag = reinterpret_cast<unsigned long long *>(im->d_small + nblk);
    x.stamp = 0x8000000000000000ull | ++im->small_seq;
    x.full_H = im->full_H; x.win_y0 = im->win_y0;
    x.consts = im->d_small_consts;
    {
        int mul = (int)(nblk_band * 0.381966) | 1;
        auto gcd = [](int a, int b) { while (b) { int t = a % b; a = b; b = t; } return a; };
        while (mul > 1 && gcd(mul, nblk_band) != 1) mul += 2;
        if (nblk_band < 4) mul = 1;
        x.perm_mul = mul % nblk_band ? mul % nblk_band : 1;
        x.perm_add = nblk_band / 3 + 1;
    }
    // (Dealing the tiles to the block slots by the star counts of the call before -- heaviest first, each to the free slot of
    // its band whose CU holds the least -- was built on top of the shuffle and measured 23.1-23.3 us against 23.4-23.7: a
    // block's duration correlates with its star count at 0.3 only.  Removed.)
    x.stamps = nullptr;
    static const char *stamp_path = getenv("CEL_SMALL_STAMPS");     // diagnostic: dump every block's phase stamps of each call
    DevBuf<unsigned long long> d_stamps;
    if (stamp_path) { HIP_TRY(d_stamps.grow(8 * nblk, 8 * nblk, st)); x.stamps = d_stamps; }
    int pi = prof_slot(c, CEL_K_SMALL_STARS);
    LAUNCH_EV(k_small_stars, dim3((unsigned)nblk), dim3(64 * SMALL_NWV), st, EV0(c, pi), EV1(c, pi), a, x);
    const bool ll = (flags & CEL_RENDER_LOGLIK) != 0;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    if (d_stamps) {
        std::vector<unsigned long long> hs((size_t)8 * nblk);
        (void)hipMemcpy(hs.data(), d_stamps, sizeof(unsigned long long) * 8 * nblk, hipMemcpyDeviceToHost);
        if (FILE *fp = fopen(stamp_path, "wb")) { fwrite(hs.data(), sizeof(unsigned long long), hs.size(), fp); fclose(fp); }
    }
    unsigned long long cur0;
    memcpy(&cur0, im->h_small + nblk, sizeof(cur0));
    if (cur0 == x.stamp) { im->small_off = true; im->records_written(0, S); return CEL_OK; }    // (it wrote a part of the tables)
    if (ll) {
        // a band's partials in a fixed order -- eight interleaved Kahan sums (index mod 8: independent chains for the host's
        // pipeline; one chain of 512 dependent adds per band was 13 us of the step), added in order: the same bits
        // whatever order the blocks ran in
        for (int b = 0; b < B; b++) {
            const double *pb = im->h_small + (size_t)b * nblk_band;
            double sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, comp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int i = 0;
            for (; i + 8 <= nblk_band; i += 8)
                for (int k = 0; k < 8; k++) {
                    const double y = pb[i + k] - comp[k];
                    const double t = sum[k] + y;
                    comp[k] = (t - sum[k]) - y;
                    sum[k] = t;
                }
            for (int k = 0; i < nblk_band; i++, k++) {
                const double y = pb[i] - comp[k];
                const double t = sum[k] + y;
                comp[k] = (t - sum[k]) - y;
                sum[k] = t;
            }
            c->mail->ll_band[b] = ((sum[0] + sum[1]) + (sum[2] + sum[3])) + ((sum[4] + sum[5]) + (sum[6] + sum[7]));
            im->h_llband[b] = c->mail->ll_band[b];
        }
        im->llband_on_host = true;              // d_llband does not hold this render's sums (cel_images_loglik_device uploads them)
    }
    im->small_star_render(src->gen, S, !(flags & CEL_RENDER_NO_STORE));
    im->last_entries = 0;
    *done = true;
    return CEL_OK;
}

// What one render does, decided once from (context, images, sources, flags, lambda_out) before anything is queued.
struct RenderPlan {
    int flags;                      // the caller's, without the internal CEL_RENDER_KEEP_LISTS
    bool keep_lists, own_rows;      // own_rows: the image set owns a part of its rows (cel_images_set_noise_rows) ...
    int own_ty0, own_ty1;           // ... the tile rows a log-likelihood adds
    bool diag, stars_only;          // the kernel: the instantiation with counters / time stamps / ablations; the star-tile kernel
    bool small_stars, incremental;  // may be TRIED: the one-launch path of a small star field; the incremental render (the changed rows decide)
    int parts, parts_used;          // blocks per tile launched; what the image vouches for (0: the star-tile kernel's bits)
    int tile_order;
    bool bin_direct;
    bool masked_ll;                 // a masked set's log-likelihood: the render without its Poisson term, then k_masked_ll (k_mask.h)
};

static int plan_render(const cel_images *im, const cel_sources *src, int flags, const double *lambda_out, RenderPlan &p) {
    const cel_ctx *c = im->ctx;
    const int64_t S = src->S;
    const int T = im->B * im->ntx * im->nty;
    p.keep_lists = (flags & CEL_RENDER_KEEP_LISTS) != 0;
    p.flags = flags &= ~CEL_RENDER_KEEP_LISTS;
    // a MASKED set: the kernel this render would have chosen anyway renders the model image; the Poisson term is a pass of its
    // own over the STORED image (CEL_RENDER_NO_STORE stores anyway: the same values, bit for bit)
    p.masked_ll = im->any_masked && (flags & CEL_RENDER_LOGLIK) && !lambda_out;
    if (p.masked_ll) p.flags = flags &= ~CEL_RENDER_NO_STORE;
    // the rows this image set OWNS (cel_images_set_noise_rows; default: all): the log-likelihood adds their tiles only
    p.own_rows = im->noise_y0 > 0 || im->noise_y1 < im->H;
    p.own_ty0 = 0; p.own_ty1 = im->nty;
    if (p.own_rows && (flags & CEL_RENDER_LOGLIK)) {
        if (im->noise_y0 % im->TH != 0 || (im->noise_y1 % im->TH != 0 && im->noise_y1 < im->H))
            return fail(CEL_ERR_INVALID, "the owned rows [%d, %d) must begin and end on render-tile rows (%d) for a log-likelihood",
                        im->noise_y0, im->noise_y1, im->TH);
        p.own_ty0 = im->noise_y0 / im->TH;
        p.own_ty1 = std::min(im->nty, (im->noise_y1 + im->TH - 1) / im->TH);
    }
    // a catalogue without galaxies: the star-tile kernel (k_render_stars.h), when the frame has more tiles than the
    // general kernel has wave slots (STAR_TILES_MIN; measured break-even, tools/star_tiles_threshold.py); the
    // instantiation with counters / time stamps / ablations exists for the general kernel only
    p.diag = c->tile_timing || (c->debug & ~64);
    const bool stars = im->TW == HW_TW && !p.diag && c->variant != 0 && src->n_gal == 0 && im->star_one_segment;
    p.stars_only = stars && c->star_tiles && (c->star_tiles == 2 || T > STAR_TILES_MIN);    // (1 and 3: the rule; 3 = without the one-launch small path)
    // a small star field (configs[1]): one launch instead of four (k_small_stars.h) -- unless a caller needs the tile lists
    // (the photon split, the E-step), an image of its own or the diagnostics
    p.small_stars = stars && S > 0 && S <= SMALL_MAX_S && T <= STAR_TILES_MIN && c->star_tiles == 1 && !im->small_off && !lambda_out &&
                    !p.keep_lists && !(flags & CEL_RENDER_STRICT) && !p.own_rows;
    p.parts = p.diag ? 1 : tile_parts_of(c, im);
    p.parts_used = (im->TW == HW_TW && !p.diag) ? p.parts : 1;
    if (p.stars_only) p.parts_used = 0;         // (the star-tile kernel adds a pixel's stars in another order: not the general kernel's bits)
    p.incremental = c->incremental && !lambda_out && !(flags & (CEL_RENDER_NO_STORE | CEL_RENDER_STRICT)) && im->TW == HW_TW &&
                    c->variant != 0 && !p.diag && !p.stars_only && p.parts == 1 && S > 0 &&
                    im->incremental_base(*src, S, c->render_T, (flags & CEL_RENDER_LOGLIK) && !p.masked_ll);
    // (masked: the dirty tiles' PIXELS are rendered incrementally, every tile's partial is formed again -- no partials are kept)
    p.tile_order = tile_order_of(c, im);
    // a small catalogue is binned by one wave per tile into per-tile segments of S entries (k_bin_direct)
    p.bin_direct = S > 0 && S <= BIN_DIRECT_MAX_S && (int64_t)T * S <= ((int64_t)1 << 25);
    return CEL_OK;
}

// the fine binning kernel: the one-kernel form (first event e0) or the second half of the two-level form
static void launch_bin_fine(cel_ctx *c, cel_images *im, int64_t S, int NS, bool one_level, hipEvent_t e0, hipEvent_t e1, const BinStep &bs) {
    auto go = [&](auto kernel, int waves) {
        LAUNCH_EV(kernel, dim3(NS), dim3(64 * waves), c->stream, e0, e1,
                  im->d_boxes, im->d_kind, S, im->ntx, im->nty, im->TH, im->TW,
                  im->nsx, im->nsy, im->d_sup_cnt, im->d_sup_off, im->d_clist, im->d_clist.cap, im->d_tile_cnt,
                  im->d_tile_nstar, im->d_tile_work, im->d_tile_off, im->d_cursor, im->d_lists, im->d_lists.cap,
                  (int *)(im->d_cursor + 1), (int *)(im->d_cursor + 3), bs);
    };
    // (16-wave blocks while every super-tile gets a CU of its own, 8-wave blocks -- two to a CU -- beyond that: k_bin2.h)
    const bool small_blocks = NS > c->n_cu;
    if (!one_level) { if (small_blocks) go(k_bin_fine_blk<false, 8>, 8); else go(k_bin_fine_blk<false, 16>, 16); }
    else { if (small_blocks) go(k_bin_fine_blk<true, 8>, 8); else go(k_bin_fine_blk<true, 16>, 16); }
}

// the render kernel of the image set's tile layout and the plan
// comps != nullptr: the general one-block kernel on the component cache (the caller has checked that the plan is that kernel's)
static void launch_render(cel_ctx *c, const cel_images *im, const RenderPlan &p, int T, const RenderArgs &a, hipEvent_t e0, hipEvent_t e1,
                          const double *comps = nullptr) {
    hipStream_t st = c->stream;
    if (im->TW == QW_TW)
        LAUNCH_EV(k_render_qw, dim3(T), dim3(64), st, e0, e1, a);
    else if (im->TW == HW_TW) {
        // the production instantiation has no diagnostic code in it; counters, time stamps and (CEL_ABLATE
        // builds) ablations live in the second one
        if (p.diag) LAUNCH_EV(k_render_hw<true>, dim3(T), dim3(64), st, e0, e1, a);
        else if (p.stars_only) LAUNCH_EV((k_render_stars<2, false>), dim3(T), dim3(64), st, e0, e1, a);
        else if (p.parts > 1) {
            const unsigned grid = (unsigned)(((T + 7) / 8) * 8 * p.parts);
            if (p.parts == 4) LAUNCH_EV((k_render_hw<false, 4>), dim3(grid), dim3(64), st, e0, e1, a);
            else LAUNCH_EV((k_render_hw<false, 2>), dim3(grid), dim3(64), st, e0, e1, a);
        }
        else if (comps) LAUNCH_EV(k_render_hwc, dim3(T), dim3(64), st, e0, e1, a, comps);
        else LAUNCH_EV(k_render_hw<false>, dim3(T), dim3(64), st, e0, e1, a);
    }
    else if (im->TH == 64)
        LAUNCH_EV((k_render<64>), dim3(T), dim3(64), st, e0, e1, a);
    else
        LAUNCH_EV((k_render<32>), dim3(T), dim3(64), st, e0, e1, a);
}

// a masked set's Poisson term: one partial per render tile from the stored image (k_mask.h), added by k_reduce in its fixed order
static void launch_masked_ll(cel_ctx *c, cel_images *im, const RenderPlan &p) {
    const int T = im->B * im->ntx * im->nty;
    int pi = prof_slot(c, CEL_K_MASKED_LL);
    LAUNCH_EV(k_masked_ll, dim3(T), dim3(64), c->stream, EV0(c, pi), EV1(c, pi), (const double *)im->d_nelec, (const double *)im->d_lambda,
              im->H, im->W, im->TW, im->TH, im->ntx, im->nty, im->d_partials.get());
    pi = prof_slot(c, CEL_K_REDUCE);
    LAUNCH_EV(k_reduce, dim3(im->B), dim3(256), c->stream, EV0(c, pi), EV1(c, pi), (const double *)im->d_partials, im->ntx * im->nty, im->d_llband.get(),
              im->ntx, p.own_ty0, p.own_ty1);
    im->llband_on_host = false;
    im->partials_overwritten();     // (nothing vouches for these partials between renders: a masked render forms every one again)
}

// the bands' sums in the mailbox, handed to the caller
static void ll_from_mailbox(const cel_ctx *c, int B, double *ll_band, double *ll_total) {
    double tot = 0.0;
    for (int b = 0; b < B; b++) {
        if (ll_band) ll_band[b] = c->mail->ll_band[b];
        tot += c->mail->ll_band[b];
    }
    if (ll_total) *ll_total = tot;
}

static int render_impl(cel_images *im, cel_sources *src, int flags, double *ll_band, double *ll_total, double *lambda_out) {
    if (!im || !src) return fail(CEL_ERR_INVALID, "cel_render_field: null argument");
    if (src->ctx != im->ctx) return fail(CEL_ERR_INVALID, "images and sources belong to different contexts");
    if (src->B != im->B) return fail(CEL_ERR_INVALID, "sources carry %d bands, images %d", src->B, im->B);
    if ((ll_band || ll_total) && !(flags & CEL_RENDER_LOGLIK))
        return fail(CEL_ERR_INVALID, "log-likelihood outputs requested without CEL_RENDER_LOGLIK");
    if ((flags & CEL_RENDER_LOGLIK) && !im->have_nelec)
        return fail(CEL_ERR_INVALID, "CEL_RENDER_LOGLIK needs cel_images_set_nelec first");
    cel_ctx *c = im->ctx;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int64_t S = src->S;
    const int T = im->B * im->ntx * im->nty;
    int rc;
    RenderPlan plan;
    if ((rc = plan_render(im, src, flags, lambda_out, plan))) return rc;
    flags = plan.flags;
    if (plan.small_stars) {
        bool done = false;
        if ((rc = render_small_stars(im, src, plan.masked_ll ? (flags & ~CEL_RENDER_LOGLIK) : flags, &done))) return rc;
        if (done) {
            if (plan.masked_ll) {
                launch_masked_ll(c, im, plan);
                HIP_TRY(hipMemcpyAsync(c->mail->ll_band, im->d_llband, sizeof(double) * im->B, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipStreamSynchronize(st));
            }
            if (flags & CEL_RENDER_LOGLIK) ll_from_mailbox(c, im->B, ll_band, ll_total);
            return CEL_OK;
        }
    }
    // The INCREMENTAL render (round 5).  The reference's single-source moves (util/infer/mcmc_transitions.py:37-152) evaluate the
    // whole field's likelihood after changing ONE source.  When this image set still holds the model image, records, lists and
    // per-tile Poisson partials of an earlier generation of THIS catalogue and only a few rows changed since
    // (cel_sources_set_rows stamps them), only the tiles that the changed sources' boxes touch -- the boxes they had and the
    // boxes they have now -- are rendered again, each from its complete list: the same arithmetic in the same order as the full
    // render, so pixels, partials and log-likelihoods are the full render's bit for bit; every other tile's pixels and partial
    // are still valid.  Source preparation runs in full (27 us at configs[2]), the binning only when the move changed a box or
    // a kind (below); a render with nothing changed, or after a whole-catalogue upload, renders every tile -- no pixel, partial
    // or log-likelihood is ever answered from a cache.
    DeltaRows delta;
    delta.n = 0;
    bool incr = plan.incremental;
    auto mark_dirty = [&] {
        hipLaunchKernelGGL(k_mark_dirty, dim3((unsigned)((delta.n * im->B + 255) / 256)), dim3(256), 0, st, delta, (const int4 *)im->d_boxes, S, im->B,
                           im->ntx, im->nty, im->TW, im->TH, im->d_dirty);
    };
    if (incr) {
        for (int64_t s = 0; s < S && incr; s++)
            if (src->row_gen[(size_t)s] > im->model.lambda_gen) {
                if (delta.n == DELTA_MAX) incr = false;
                else delta.idx[delta.n++] = (int)s;
            }
        if (delta.n == 0) incr = false;
    }
    if (incr) {
        HIP_TRY(im->d_dirty.grow(T, T, st));
        HIP_TRY(hipMemsetAsync(im->d_dirty, 0, sizeof(int) * (size_t)T, st));
        mark_dirty();   // the tiles the changed sources' OLD boxes touch (before k_prep rewrites the boxes) ...
    }
    // Binning only when a box or a kind changed.  The tile lists are a function of the (box, kind) table, the tiling and the
    // source count alone -- no flux enters them.  When the host vouches that the lists stand for the table in d_boxes /
    // d_kind (binning_of, asked BEFORE this render's k_prep fires records_written), k_prep compares what it is about to store
    // with that table ON THE DEVICE, on every call, and the binning kernels return at once unless it found a difference.
    // CEL_OPT_INCREMENTAL = 0: no comparison, the binning runs in full.
    bool bins_stand = c->incremental && im->lists.binning_of(S);
    // No source preparation when the records stand as well.  The records are a function of the catalogue's rows, the bands' WCS
    // and PSF tables, the window and the source count; when the tables hold those of exactly this generation and the last
    // render binned its lists from them (prep_stands, asked BEFORE render_begins drops lists_gen), k_prep would store what
    // stands there and find nothing to change: it is not launched, and the binning launch leaves every word as it is
    // (BIN_LEAVE).  A new sky level, new pixels, a log-likelihood after a plain render, a call that read the boxes in between:
    // all render from the records in place.  Every tile is rendered all the same.
    bool recs_stand = im->prep_stands(*src, S, c->incremental != 0);
    im->render_begins((flags & CEL_RENDER_LOGLIK) != 0, !lambda_out && !(flags & CEL_RENDER_NO_STORE));
    // (the list buffers first: one that had to be re-allocated holds no lists, whatever the stamps said)
    const int64_t lists_cap0 = im->d_lists.cap, clist_cap0 = im->d_clist.cap;
    if (im->d_lists.cap == 0) {
        // first guess: every (band, source) touches ~6 tiles; grown on overflow below
        const int64_t n = (S * im->B) * 6 + 1024;
        HIP_TRY(im->d_lists.grow(n, n, st));
    }
    if (im->d_clist.cap == 0) {
        // first guess: every (band, source) touches ~3 super-tiles; grown on overflow below
        const int64_t n = (S * im->B) * 3 + 1024;
        HIP_TRY(im->d_clist.grow(n, n, st));
    }
    const int NS = im->B * im->nsx * im->nsy;
    const int tile_order = plan.tile_order, parts = plan.parts;
    const bool bin_direct = plan.bin_direct, diag = plan.diag;
    if (bin_direct) HIP_TRY(im->d_lists.grow((int64_t)T * S, (int64_t)T * S, st));
    if (im->d_lists.cap != lists_cap0 || im->d_clist.cap != clist_cap0) { im->lists_regrown(); bins_stand = recs_stand = false; }
    if (!recs_stand) {
        rc = run_prep(im, src, nullptr, 0, bins_stand ? ++im->bin_step : 0ull);
        if (rc) return rc;
    }
    if (incr) mark_dirty();     // ... and the tiles their new boxes touch
    // The component cache (k_comps.h).  A render that launched no k_prep reads records that stand from call to call: what a
    // tile entry's set-up computes from its record alone is built once per record generation, in front of the first such
    // render, and loaded by this and every later one (k_render_hwc) until an event disowns the records.  A render whose k_prep
    // ran takes the plain kernel and leaves the cache stale (records_written): the dirty-tile render, the chain that moves
    // every source and the whole upload run exactly the code they ran without it.
    const double *comps = nullptr;
    if (recs_stand && c->comp_cache && im->TW == HW_TW && !diag && !plan.stars_only && parts == 1 && c->variant != 0 && S > 0) {
        const int64_t n_rec = S * im->B;
        const int64_t cap0 = im->d_comps.cap;
        HIP_TRY(im->d_comps.grow(n_rec * COMP_ROW, n_rec * COMP_ROW + n_rec * COMP_ROW / 4, st));
        if (im->d_comps.cap != cap0 || !im->rec.comps_of_records()) {      // (a block just allocated holds nobody's rows)
            int pi = prof_slot(c, CEL_K_GMM);
            LAUNCH_EV(k_comps, dim3((unsigned)((n_rec + COMPS_WAVES - 1) / COMPS_WAVES)), dim3(64 * COMPS_WAVES), st, EV0(c, pi), EV1(c, pi),
                      (const BandDev *)im->d_bands, (const SrcRec *)im->d_recs, S, n_rec, im->d_comps.get());
            HIP_TRY(hipGetLastError());
            im->comps_built();
        }
        comps = im->d_comps;
    }
    for (int attempt = 0; attempt < 8; attempt++) {
        // (a retry bins: its cursor words were zeroed by hand, the attempt before it left half-built lists)
        const BinStep bs = {im->d_cursor, im->bin_step, attempt > 0 ? BIN_ALWAYS : (recs_stand ? BIN_LEAVE : (bins_stand ? BIN_IF_CHANGED : BIN_ALWAYS))};
        // d_cursor: [0] fine cursor, [1] fine overflow, [2] coarse cursor, [3] coarse overflow;
        // zeroed by k_prep (no memset in the queue), by hand only for an empty catalogue or on a retry; a render that launched
        // no k_prep (recs_stand) leaves them as the binning that built the lists left them
        if (attempt > 0 || S * im->B == 0) HIP_TRY(hipMemsetAsync(im->d_cursor, 0, sizeof(unsigned long long) * 4, st));
        // one event pair over the binning kernels: start on the first, stop on the last
        int pi = prof_slot(c, CEL_K_BIN);
        // the order by the previous render's measured durations was sorted behind that render's readback
        // (below): nothing to do here then
        const bool order_ready = tile_order == 1 && im->lists.order_ready(S);
        const hipEvent_t bin_ev1 = (tile_order && !order_ready) ? (hipEvent_t) nullptr : EV1(c, pi);
        // a small catalogue: one wave per tile (k_bin_direct).  Otherwise one binning kernel while no super-tile holds more
        // than BIN_CH candidates, the two-level form after that
        if (bin_direct) {
            LAUNCH_EV(k_bin_direct, dim3(T), dim3(64), st, EV0(c, pi), bin_ev1, im->d_boxes, im->d_kind, S, im->ntx, im->nty, im->TH, im->TW,
                      im->d_tile_cnt, im->d_tile_nstar, im->d_tile_work, im->d_tile_off, im->d_cursor, im->d_lists, bs);
        } else if (im->bin_two_level) {
            LAUNCH_EV(k_bin_coarse, dim3(NS), dim3(64 * COARSE_WAVES), st, EV0(c, pi), (hipEvent_t) nullptr, im->d_boxes, S, im->nsx, im->nsy,
                      im->d_sup_cnt, im->d_sup_off, im->d_cursor + 2, im->d_clist, im->d_clist.cap, (int *)(im->d_cursor + 3), bs);
            launch_bin_fine(c, im, S, NS, false, (hipEvent_t) nullptr, bin_ev1, bs);
        } else {
            launch_bin_fine(c, im, S, NS, true, EV0(c, pi), bin_ev1, bs);
        }
        if (tile_order && !order_ready)
            // heaviest first: by the durations the tiles had in the previous render when that was
            // of the same source count (an MCMC chain changes little from one evaluation to the
            // next), by the binning pass's estimate otherwise.  The order never changes results.
            LAUNCH_EV(k_order, dim3(1), dim3(1024), st, (hipEvent_t) nullptr, EV1(c, pi),
                      (const int *)((im->lists.costs_of(S) && tile_order == 1) ? im->d_tile_cost : im->d_tile_work), T, im->d_order);
        RenderArgs a;
        a.bands = im->d_bands; a.recs = im->d_recs; a.lists = im->d_lists; a.tile_cnt = im->d_tile_cnt;
        a.tile_nstar = im->d_tile_nstar;
        a.tile_off = im->d_tile_off; a.nelec = im->d_nelec; a.lambda = lambda_out ? lambda_out : im->d_lambda; a.partials = im->d_partials;
        a.S = S; a.capacity = im->d_lists.cap; a.B = im->B; a.H = im->H; a.W = im->W; a.ntx = im->ntx; a.nty = im->nty;
        a.flags = (plan.masked_ll ? (flags & ~CEL_RENDER_LOGLIK) : flags) | (c->debug << 8); a.variant = c->variant; a.tail_T = c->render_T; a.order = tile_order ? im->d_order : nullptr;
        a.timing = nullptr;
        a.dirty = incr ? im->d_dirty : nullptr;
        a.cost = (im->TW == HW_TW || im->TW == QW_TW) ? im->d_tile_cost : nullptr;
        if (c->tile_timing) {
            HIP_TRY(im->d_timing.grow(3 * T, 3 * T, st));
            a.timing = im->d_timing;
        }
        a.slabs = nullptr; a.part_cnt = nullptr;
        if (parts > 1) {
            const int64_t slabs = (int64_t)HW_TH * HW_TW * T * parts;
            HIP_TRY(im->d_slabs.grow(slabs, slabs, st));
            if (!im->d_part_cnt) {
                HIP_TRY(im->d_part_cnt.grow(T, T, st));
                HIP_TRY(hipMemsetAsync(im->d_part_cnt, 0, sizeof(int) * (size_t)T, st));
            }
            a.slabs = im->d_slabs; a.part_cnt = im->d_part_cnt;
        }
        pi = prof_slot(c, plan.stars_only ? CEL_K_RENDER_STARS : CEL_K_RENDER);
        launch_render(c, im, plan, T, a, EV0(c, pi), EV1(c, pi), comps);
        if (plan.masked_ll) launch_masked_ll(c, im, plan);
        else if (flags & CEL_RENDER_LOGLIK) {
            pi = prof_slot(c, CEL_K_REDUCE);
            LAUNCH_EV(k_reduce, dim3(im->B), dim3(256), st, EV0(c, pi), EV1(c, pi), (const double *)im->d_partials, im->ntx * im->nty, im->d_llband,
                      im->ntx, plan.own_ty0, plan.own_ty1);
            im->llband_on_host = false;
        }
        // the per-band sums, the total list length and the overflow flags ride back in ONE copy
        HIP_TRY(hipMemcpyAsync(c->mail.get(), im->d_llband, offsetof(Mailbox, sh) + sizeof(MailShared::bin_coarse),
                               hipMemcpyDeviceToHost, st));
        HIP_TRY(hipGetLastError());
        // An MCMC chain renders the same number of sources again: sort this render's tile durations into
        // the next render's launch order NOW, behind the readback the host is waiting for, instead of
        // in front of the next render (13 us + a launch gap per step).  The host waits for the copy only.
        const bool post_order = (tile_order == 1 && a.cost != nullptr);
        if (post_order) {
            if (!im->ev_step) HIP_TRY(hipEventCreateWithFlags(&im->ev_step, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(im->ev_step, st));
            hipLaunchKernelGGL(k_order, dim3(1), dim3(1024), 0, st, (const int *)im->d_tile_cost, T, im->d_order);
            HIP_TRY(hipEventSynchronize(im->ev_step));
        } else {
            HIP_TRY(hipStreamSynchronize(st));
        }
        const unsigned long long *fine = c->mail->bin_fine, *coarse = c->mail->sh.bin_coarse;      // cursor, overflow
        const bool fine_ok = (fine[1] & 0xffffffffull) == 0 && (int64_t)fine[0] <= im->d_lists.cap;
        const bool too_dense = (coarse[1] & 2ull) != 0;        // a super-tile with more candidates than the one-kernel form stages
        const bool coarse_ok = (coarse[1] & 0xffffffffull) == 0 && (int64_t)coarse[0] <= im->d_clist.cap;
        if (coarse_ok) im->last_entries = (double)fine[0];
        if (fine_ok && coarse_ok) {
            // a render by the DIAG instantiation (tile timing, ablation bits) vouches for nothing (0 parts): with an ablation bit
            // set its pixels and partials are documented as wrong, and the incremental path would take them as a base
            // (last_dirty: counted on request, cel_debug_last_render)
            im->render_succeeded(*src, S, a.cost != nullptr, post_order,
                                 !lambda_out && !(flags & (CEL_RENDER_NO_STORE | CEL_RENDER_STRICT)) && im->TW == HW_TW && c->variant != 0,
                                 c->render_T, diag ? 0 : plan.parts_used, (flags & CEL_RENDER_LOGLIK) && !plan.masked_ll, incr);
            break;
        }
        im->render_overflowed();
        // rerun with room (a truncated coarse list also truncates the fine counts)
        if (too_dense) { im->bin_two_level = true; im->bin_form_changed(); continue; }
        const int64_t nc = (int64_t)coarse[0] + (int64_t)coarse[0] / 4 + 1024, nf = (int64_t)fine[0] + (int64_t)fine[0] / 4 + 1024;
        if (!coarse_ok) HIP_TRY(im->d_clist.grow(nc, nc, st));
        if (!fine_ok) HIP_TRY(im->d_lists.grow(nf, nf, st));
        im->lists_regrown();
        if (attempt == 7) return fail(CEL_ERR_HIP, "tile lists kept overflowing");
    }
    if (flags & CEL_RENDER_LOGLIK) ll_from_mailbox(c, im->B, ll_band, ll_total);
    return CEL_OK;
}

int cel_debug_split_rates(cel_images *im, double *out) {
    if (!im || !out) return fail(CEL_ERR_INVALID, "cel_debug_split_rates: null argument");
    if (!im->d_rate) return fail(CEL_ERR_INVALID, "no totals image: cel_photon_split on the recurrence kernels has not run");
    HIP_TRY(hipSetDevice(im->ctx->device));
    return copy_out(out, im->split.rate_in_lambda ? im->d_lambda : im->d_rate, sizeof(double) * (size_t)im->B * im->H * im->W, CEL_HOST, im->ctx->stream);
}

int cel_debug_last_render(cel_images *im, int64_t *dirty_tiles) {
    if (!im || !dirty_tiles) return fail(CEL_ERR_INVALID, "cel_debug_last_render: null argument");
    *dirty_tiles = -1;
    if (im->model.last_dirty == -1 || !im->d_dirty) return CEL_OK;
    HIP_TRY(hipSetDevice(im->ctx->device));
    const int T = im->B * im->ntx * im->nty;
    std::vector<int> h((size_t)T);
    int rc = copy_out(h.data(), im->d_dirty, sizeof(int) * (size_t)T, CEL_HOST, im->ctx->stream);
    if (rc) return rc;
    int64_t n = 0;
    for (int v : h) n += (v != 0);
    *dirty_tiles = n;
    return CEL_OK;
}

int cel_debug_tile_timing(cel_images *im, uint64_t *out, int64_t *n_tiles) {
    if (!im || !n_tiles) return fail(CEL_ERR_INVALID, "cel_debug_tile_timing: null argument");
    const int T = im->B * im->ntx * im->nty;
    *n_tiles = T;
    if (!out) return CEL_OK;
    if (!im->d_timing) return fail(CEL_ERR_INVALID, "no timing recorded: set CEL_OPT_TILE_TIMING before rendering");
    HIP_TRY(hipSetDevice(im->ctx->device));
    return copy_out(out, im->d_timing, sizeof(unsigned long long) * 3 * T, CEL_HOST, im->ctx->stream);
}

int cel_field_stats(cel_images *im, double *n_srcpix, double *n_gauss, double *n_tile_entries) {
    if (!im) return fail(CEL_ERR_INVALID, "null images");
    cel_ctx *c = im->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int64_t n = im->rec.last_S * im->B;
    HIP_TRY(hipMemsetAsync(im->d_stats, 0, sizeof(double) * 2, c->stream));
    if (n > 0)
        hipLaunchKernelGGL(k_stats, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, im->d_recs, n, im->d_stats);
    HIP_TRY(hipMemcpyAsync(c->mail->sh.w.field_stats, im->d_stats, sizeof(double) * 2, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n_srcpix) *n_srcpix = c->mail->sh.w.field_stats[0];
    if (n_gauss) *n_gauss = c->mail->sh.w.field_stats[1];
    if (n_tile_entries) *n_tile_entries = im->last_entries;
    return CEL_OK;
}

// ---- stamps ---------------------------------------------------------------------------------
// prep for ONE band: records are laid out [band][source]; the band's slice is reused.
int cel_stamp_boxes(cel_images *im, cel_sources *src, int band, int32_t *boxes, int32_t *status) {
    if (!im || !src || !boxes || !status) return fail(CEL_ERR_INVALID, "cel_stamp_boxes: null argument");
    if (band < 0 || band >= im->B) return fail(CEL_ERR_INVALID, "band %d out of range", band);
    if (src->B != im->B || src->ctx != im->ctx) return fail(CEL_ERR_INVALID, "sources do not match images");
    cel_ctx *c = im->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc = host_boxes(im, src);
    if (rc) return rc;
    const int64_t S = src->S;
    const int4 *hb = im->h_boxes.data() + (int64_t)band * S;     // x0, x1, y0, y1
    const int *hs = im->h_status.data() + (int64_t)band * S;
    for (int64_t s = 0; s < S; s++) {
        boxes[4 * s + 0] = hb[s].z; boxes[4 * s + 1] = hb[s].w;
        boxes[4 * s + 2] = hb[s].x; boxes[4 * s + 3] = hb[s].y;
        status[s] = hs[s];
    }
    return CEL_OK;
}

int cel_render_stamps(cel_images *im, cel_sources *src, int band, int scaled, const int32_t *boxes_in,
                      const int64_t *offsets, double *out, int mem) {
    if (!im || !src || !offsets || !out) return fail(CEL_ERR_INVALID, "cel_render_stamps: null argument");
    if (band < 0 || band >= im->B) return fail(CEL_ERR_INVALID, "band %d out of range", band);
    if (src->B != im->B || src->ctx != im->ctx) return fail(CEL_ERR_INVALID, "sources do not match images");
    if (scaled < 0 || scaled > 3)
        return fail(CEL_ERR_INVALID, "cel_render_stamps: scaled must be 0, 1 (stamps) or 2, 3 (derivative planes), not %d", scaled);
    const bool jac = scaled >= 2;              // k_stamp_jac.h: the stamp and its parameter derivatives, 3 or 7 planes per source
    cel_ctx *c = im->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int64_t S = src->S;
    if (S == 0) return CEL_OK;
    if (offsets[0] != 0) return fail(CEL_ERR_INVALID, "cel_render_stamps: offsets[0] must be 0");
    // the planes of a slot follow the source's type: the host's copy of the types, read back where the device wrote them last
    std::vector<int32_t> types_now;
    if (jac && (int64_t)src->h_type.size() != S) {
        types_now.resize((size_t)S);
        HIP_TRY(hipMemcpyAsync(types_now.data(), src->d_type, sizeof(int) * S, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    const int32_t *h_type = !jac ? nullptr : (types_now.empty() ? src->h_type.data() : types_now.data());
    std::vector<int32_t> hb((size_t)S * 4), hs((size_t)S);
    int rc = cel_stamp_boxes(im, src, band, hb.data(), hs.data());
    if (rc) return rc;
    std::vector<int4> obox((size_t)S);
    std::vector<StampJob> jobs;
    std::vector<int64_t> skipped;   // sources without a stamp whose slot in `out` is not empty
    const int ROWS = 64;
    const int strip_w = (c->variant == 0) ? TILE_W : HW_TW;     // the recurrence kernel works on 32 x 64 chunks
    for (int64_t s = 0; s < S; s++) {
        int y0, y1, x0, x1;
        bool ok;
        if (boxes_in) {
            y0 = boxes_in[4 * s]; y1 = boxes_in[4 * s + 1]; x0 = boxes_in[4 * s + 2]; x1 = boxes_in[4 * s + 3];
            ok = (y1 > y0 && x1 > x0) && hs[s] != -1;   // an overlap-test miss is None whatever the limits
        } else {
            y0 = hb[4 * s]; y1 = hb[4 * s + 1]; x0 = hb[4 * s + 2]; x1 = hb[4 * s + 3];
            ok = hs[s] > 0;
        }
        obox[s] = make_int4(x0, x1, y0, y1);
        if (offsets[s + 1] < offsets[s]) return fail(CEL_ERR_INVALID, "offsets must not decrease (source %lld)", (long long)s);
        if (!ok) {
            // the reference returns (None, None, None) here; the slot the caller sized for it is
            // zero-filled so that nothing stale can be read from it
            if (offsets[s + 1] > offsets[s]) skipped.push_back(s);
            continue;
        }
        int64_t area = (int64_t)(y1 - y0) * (x1 - x0);
        const int planes = !jac ? 1 : ((h_type[s] == 1 || h_type[s] == 2) ? 7 : 3);
        if (offsets[s + 1] - offsets[s] != planes * area)
            return fail(CEL_ERR_INVALID, "offsets[%lld+1]-offsets[%lld] = %lld but the stamp has %d plane(s) of %lld pixels",
                        (long long)s, (long long)s, (long long)(offsets[s + 1] - offsets[s]), planes, (long long)area);
        for (int xs = x0; xs < x1; xs += strip_w)
            for (int ys = y0; ys < y1; ys += ROWS)
                jobs.push_back(StampJob{(int)s, xs, ys, ys + ROWS < y1 ? ys + ROWS : y1});
    }
    int64_t total = offsets[S];
    if (jobs.empty() && (skipped.empty() || mem != CEL_DEVICE)) {
        if (mem != CEL_DEVICE)
            for (int64_t s : skipped) memset(out + offsets[s], 0, sizeof(double) * (size_t)(offsets[s + 1] - offsets[s]));
        return CEL_OK;
    }
    StampJob *d_jobs = nullptr;
    int4 *d_obox = nullptr;
    int64_t *d_off = nullptr;
    double *d_out = nullptr;
    if ((rc = scratch_get(c, SCR_TMP_A, sizeof(StampJob) * jobs.size(), (void **)&d_jobs)) ||
        (rc = scratch_get(c, SCR_TMP_B, sizeof(int4) * S, (void **)&d_obox)) ||
        (rc = scratch_get(c, SCR_TMP_C, sizeof(int64_t) * (S + 1), (void **)&d_off)))
        return rc;
    if (mem == CEL_DEVICE) d_out = out;
    else if ((rc = scratch_get(c, SCR_HOST_IO, sizeof(double) * (total > 0 ? total : 1), (void **)&d_out))) return rc;
    for (int64_t s : skipped)
        HIP_TRY(hipMemsetAsync(d_out + offsets[s], 0, sizeof(double) * (size_t)(offsets[s + 1] - offsets[s]), c->stream));
    if (!jobs.empty()) {
        HIP_TRY(hipMemcpyAsync(d_jobs, jobs.data(), sizeof(StampJob) * jobs.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_obox, obox.data(), sizeof(int4) * S, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_off, offsets, sizeof(int64_t) * (S + 1), hipMemcpyHostToDevice, c->stream));
        int pi = prof_begin(c, CEL_K_STAMPS);
        if (jac)
            hipLaunchKernelGGL(k_stamp_jac, dim3((unsigned)jobs.size()), dim3(64), 0, c->stream, (const BandDev *)im->d_bands, band,
                               (const SrcRec *)(im->d_recs + (int64_t)band * S), (const StampJob *)d_jobs, (const int4 *)d_obox,
                               (const int64_t *)d_off, (const int *)src->d_type, (const double *)src->d_shape, im->win_y0, strip_w,
                               scaled == 3, d_out);
        else if (c->variant == 0)
            hipLaunchKernelGGL(k_stamps, dim3((unsigned)jobs.size()), dim3(64), 0, c->stream, im->d_bands, band,
                               im->d_recs + (int64_t)band * S, d_jobs, d_obox, d_off, scaled, d_out);
        else
            hipLaunchKernelGGL(k_stamps_hw, dim3((unsigned)jobs.size()), dim3(64), 0, c->stream, im->d_bands, band,
                               im->d_recs + (int64_t)band * S, d_jobs, d_obox, d_off, scaled, c->tail_T, d_out);
        prof_end(c, pi);
        HIP_TRY(hipGetLastError());
        if (mem != CEL_DEVICE) HIP_TRY(hipMemcpyAsync(out, d_out, sizeof(double) * total, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));      // (jobs, obox and the caller's arrays were the sources of asynchronous copies)
    return CEL_OK;
}

// ---- per-source conditional log-likelihoods ---------------------------------------------------
static const int CEL_PLL_GRAD = 8;      // mode = CEL_PLL_GRAD + m: the gradient form (celeste_hip.h names it in cel_patch_loglik's comment)
// cel_patch_loglik_multi in steps.  What its checks settle, then where its staging puts things:
struct PllCall {
    int mode = 0;                                   // 0, 1, 2 or 4
    bool grad = false;                              // the gradient form CEL_PLL_GRAD + mode
    bool resident = false, nzl = false;             // the resident split's patches, not a caller's; their photon lists take part
    int64_t P = 0, nb = 0;                          // proposals; (patch set, band) boxes
    std::vector<int4> hbox;                         // a caller's boxes as the kernels read them: x0, x1, y0, y1
    int nsplit = 1, nparts = 1;                     // blocks per dense job; slots per job in d_out
    int4 *d_box = nullptr, *d_nz = nullptr;
    int64_t *d_off = nullptr;
    int *d_owner = nullptr;
    double *d_data = nullptr, *d_out = nullptr;
    const int *i_data = nullptr;                    // the resident split's int32 photon counts (mode 0); everything else is double
    bool owned = true;                              // false: cel_patch_loglik's single source (its gradient keeps the dense kernel)
    // CEL_OPT_GRAD_CONDITIONAL = 1 on the resident mode 8: the exact conditional's row (k_mass_grad.h).  d_owner is then a copy the
    // cover test may retire slots in; pri holds -inf for those
    bool exact = false;
    double *d_pri = nullptr, *d_mass = nullptr, *d_exact = nullptr, *d_msums = nullptr, *d_mg = nullptr;
};
// step 1: the argument checks and the boxes.  k.P == 0 with CEL_OK: nothing to score.
static int pll_check(cel_images *im, cel_sources *src, const int32_t *owner, int64_t NB, const int32_t *boxes,
                     const int64_t *offsets, const double *data, int mode_arg, const double *ll_out, PllCall &k) {
    if (!im || !src || !ll_out) return fail(CEL_ERR_INVALID, "cel_patch_loglik: null argument");
    if (src->B != im->B || src->ctx != im->ctx) return fail(CEL_ERR_INVALID, "sources do not match images");
    // the gradient form CEL_PLL_GRAD + m, m in {0, 1, 2}: every check below is mode m's, the value in slot 0 is mode m's path
    const bool grad = k.grad = (mode_arg >= CEL_PLL_GRAD && mode_arg <= CEL_PLL_GRAD + 2);
    const int mode = k.mode = grad ? mode_arg - CEL_PLL_GRAD : mode_arg;
    if (mode != 0 && mode != 1 && mode != 2 && mode != 4)
        return fail(CEL_ERR_INVALID, "mode must be 0 (conditional), 1 (isolated), 2 (patch Poisson), 4 (Poisson on a background plane) "
                                     "or 8 + (0, 1, 2) (the gradient form)");
    // resident form: boxes == offsets == data == NULL -> the patches of the last resident photon
    // split (mode 0) or the observed image on those boxes (mode 1); NB must be that split's S
    const bool resident = k.resident = (!boxes && !offsets && !data);
    if (!resident && (!boxes || !offsets)) return fail(CEL_ERR_INVALID, "cel_patch_loglik: null boxes / offsets");
    if (resident && mode > 1) return fail(CEL_ERR_INVALID, "the resident form scores mode 0 or 1");
    const int nplanes = (mode == 4) ? 2 : 1;               // mode 4: data plane, then background plane
    // the exact conditional's gradient: the resident mode 8 of cel_patch_loglik_multi alone reads the key; it has the exact slice
    // engine's preconditions (an unmasked set, or CEL_OPT_SAMPLER_MASK; the row window is the gradient form's refusal below; the split's just below)
    k.exact = grad && mode == 0 && resident && k.owned && im->ctx->grad_conditional == 1;
    if (k.exact) { int rm = refuse_masked_sampler(im, "cel_patch_loglik_multi (resident gradient under CEL_OPT_GRAD_CONDITIONAL = 1)", true); if (rm) return rm; }
    // (a masked set is refused as such before the missing split is named: cel_images_set_nelec drops the split it masks)
    if (mode == 1) { int rm = refuse_masked(im, "cel_patch_loglik (isolated form)"); if (rm) return rm; }
    if (resident && !im->split.resident_of(NB))
        return fail(CEL_ERR_INVALID, "resident form needs a resident photon split of NB = %lld sources (have %lld)",
                    (long long)NB, (long long)im->split.samp_S);
    if (NB < 1 || (NB > 1 && !owner)) return fail(CEL_ERR_INVALID, "cel_patch_loglik: NB patch sets need an owner array");
    if (resident && mode == 1 && !im->have_nelec) return fail(CEL_ERR_INVALID, "the isolated form needs cel_images_set_nelec");
    if (grad && (im->win_y0 != 0 || im->full_H != im->H))
        return fail(CEL_ERR_INVALID, "cel_patch_loglik (gradient form): an image set with a row window (cel_images_set_window) is not supported");
    HIP_TRY(hipSetDevice(im->ctx->device));
    const int B = im->B;
    const int64_t P = k.P = src->S, nb = k.nb = NB * B;
    if (P == 0) return CEL_OK;
    if (!resident && offsets[0] != 0) return fail(CEL_ERR_INVALID, "cel_patch_loglik: offsets[0] must be 0");
    k.hbox.resize((size_t)(resident ? 0 : nb));
    for (int64_t i = 0; i < (resident ? 0 : nb); i++) {
        int y0 = boxes[4 * i], y1 = boxes[4 * i + 1], x0 = boxes[4 * i + 2], x1 = boxes[4 * i + 3];
        int64_t area = (y1 > y0 && x1 > x0) ? (int64_t)(y1 - y0) * (x1 - x0) : 0;
        if (offsets[i + 1] - offsets[i] != area * nplanes)
            return fail(CEL_ERR_INVALID, "patch set %lld band %d: offsets give %lld patch values, the box has %lld pixels x %d plane(s)",
                        (long long)(i / B), (int)(i % B), (long long)(offsets[i + 1] - offsets[i]), (long long)area, nplanes);
        if (area > 0 && (y0 < 0 || x0 < 0 || y1 > im->H || x1 > im->W))
            return fail(CEL_ERR_INVALID, "patch set %lld band %d: patch limits outside the image", (long long)(i / B), (int)(i % B));
        k.hbox[(size_t)i] = make_int4(x0, x1, y0, y1);
    }
    if (owner)
        for (int64_t p = 0; p < P; p++)
            if (owner[p] < 0 || owner[p] >= NB) return fail(CEL_ERR_INVALID, "owner[%lld] = %d out of range", (long long)p, owner[p]);
    if (!resident && offsets[nb] > 0 && !data) return fail(CEL_ERR_INVALID, "cel_patch_loglik: null data");
    return CEL_OK;
}

// step 2: the scratch slots, the carved block and the uploads -- k's device pointers are set, the copies queued
static int pll_stage(cel_images *im, const int32_t *owner, const int64_t *offsets, const double *data, int mem, PllCall &k) {
    cel_ctx *c = im->ctx;
    const int B = im->B;
    const int64_t P = k.P, nb = k.nb;
    const bool resident = k.resident;
    // a call with few proposals is a handful of one-wave jobs as long as their longest: each is dealt to PLL_PARTS blocks
    // (the values do not depend on it: the kernel sums its chunks in PLL_PARTS classes either way)
    // (with photon lists a job always owns PLL_PARTS slots: the kernel that scores at the photons writes its four class sums)
    k.nzl = resident && k.mode == 0 && c->variant != 0 && im->split.nz_valid;
    k.nsplit = (c->variant != 0 && k.mode == 0 && P * B <= 8192) ? PLL_PARTS : 1;
    k.nparts = k.nzl ? PLL_PARTS : k.nsplit;
    // one block: a caller's boxes, their photon rectangles, the owners
    auto carve = [&](char *base) {
        Carver cv{base};
        k.d_box = cv.take<int4>(resident ? 0 : nb);
        k.d_nz = cv.take<int4>(resident ? 0 : nb);
        k.d_owner = owner ? cv.take<int>(P) : nullptr;
        return cv.off;
    };
    char *d_blk = nullptr;
    int rc;
    if ((rc = scratch_get(c, SCR_PLL_BOXES, carve(nullptr), (void **)&d_blk)) ||
        (rc = scratch_get(c, SCR_OFFSETS, sizeof(int64_t) * (nb + 1), (void **)&k.d_off)) ||
        (rc = scratch_get(c, SCR_VALUES, sizeof(double) * P * B * k.nparts, (void **)&k.d_out)))
        return rc;
    carve(d_blk);
    if (owner) HIP_TRY(hipMemcpyAsync(k.d_owner, owner, sizeof(int) * P, hipMemcpyHostToDevice, c->stream));
    if (k.exact) {                   // the exact row's extras, one block: cover flags, masses, terms, the mass gradient's sums and rows
        int *d_own2 = nullptr;
        auto carve2 = [&](char *base) {
            Carver cv{base};
            k.d_pri = cv.take<double>(P);
            k.d_mass = cv.take<double>(P * B);
            k.d_exact = cv.take<double>(P);
            k.d_msums = cv.take<double>((size_t)GRAD_NS * PGRAD_PARTS * P * B);
            k.d_mg = cv.take<double>(P * (7 + B));
            d_own2 = cv.take<int>(P);
            return cv.off;
        };
        char *d_ex = nullptr;
        if ((rc = scratch_get(c, SCR_TMP_C, carve2(nullptr), (void **)&d_ex))) return rc;
        carve2(d_ex);
        if (k.d_owner) HIP_TRY(hipMemcpyAsync(d_own2, k.d_owner, sizeof(int) * P, hipMemcpyDeviceToDevice, c->stream));
        else HIP_TRY(hipMemsetAsync(d_own2, 0, sizeof(int) * P, c->stream));
        HIP_TRY(hipMemsetAsync(k.d_pri, 0, sizeof(double) * P, c->stream));
        k.d_owner = d_own2;
    }
    if (resident) {
        k.d_nz = im->d_snz; k.d_box = im->d_sbox; k.d_off = im->d_soff;
        if (k.mode == 0) k.i_data = im->d_samp;           // mode 0: the int32 patches; mode 1 reads nelec on the boxes
        return CEL_OK;
    }
    HIP_TRY(hipMemcpyAsync(k.d_box, k.hbox.data(), sizeof(int4) * nb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(k.d_off, offsets, sizeof(int64_t) * (nb + 1), hipMemcpyHostToDevice, c->stream));
    if (mem == CEL_DEVICE) { k.d_data = const_cast<double *>(data); return CEL_OK; }
    if ((rc = scratch_get(c, SCR_PATCH_DATA, sizeof(double) * (offsets[nb] > 0 ? offsets[nb] : 1), (void **)&k.d_data))) return rc;   // (copies are queued: scratch_get fails through HIP_TRY, which drains the device)
    if (offsets[nb] > 0) HIP_TRY(hipMemcpyAsync(k.d_data, data, sizeof(double) * offsets[nb], hipMemcpyHostToDevice, c->stream));
    return CEL_OK;
}

// step 3: the values, P * B * k.nparts of them in k.d_out
static void pll_launch_values(cel_images *im, const PllCall &k) {
    cel_ctx *c = im->ctx;
    const int B = im->B;
    const int64_t P = k.P;
    hipStream_t st = c->stream;
    if (c->variant == 0) {           // the direct kernel: every mode, one block and one value per job
        auto direct = [&](auto kernel, auto *z) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)(P * B)), dim3(256), 0, st, im->d_bands, B, P, im->d_recs, k.d_owner, k.d_box,
                               k.d_off, z, im->d_nelec, im->H, im->W, k.mode, k.d_out);
        };
        if (k.i_data) direct(k_patch_ll<int>, k.i_data); else direct(k_patch_ll<double>, (const double *)k.d_data);
        return;
    }
    PatchLlJob<double> jd = patch_ll_job(c, im, P, k.d_owner, k.d_out, k.d_box, k.d_off, (const double *)k.d_data);     // (no data: mode 1 on the resident boxes)
    if (k.mode == 1) launch_patch_ll<1>(c, im, jd, P * B, st);           // modes 1, 2 and 4: one block per job over the whole patch
    else if (k.mode == 2) launch_patch_ll<2>(c, im, jd, P * B, st);
    else if (k.mode == 4) launch_patch_ll<4>(c, im, jd, P * B, st);
    else if (k.i_data) {             // mode 0 on the resident split's patches
        PatchLlJob<int> j = patch_ll_job(c, im, P, k.d_owner, k.d_out, k.d_box, k.d_off, k.i_data);
        j.nzbox = k.d_nz; j.nsplit = k.nsplit; j.nzmode = k.nzl ? (const int *)im->d_nzmode : nullptr; j.ostride = k.nparts;
        launch_patch_ll<0>(c, im, j, P * B * k.nsplit, st);
        if (k.nzl)                   // ... and the proposals whose patch is scored at its photons (the others return at once)
            hipLaunchKernelGGL(k_patch_ll_nz<false>, dim3((unsigned)(P * B)), dim3(64), 0, st, im->d_bands, B, P, im->d_recs,
                               (const int *)k.d_owner, (const int4 *)k.d_box, (const int4 *)k.d_nz, (const int *)im->d_nzmode,
                               (const int64_t *)im->d_nzoff, (const NzEntry *)im->d_nzlist, k.d_out, (const int *)nullptr,
                               (const int *)nullptr, (const SliceFuse *)nullptr);
    } else {                         // mode 0 on a caller's patches: on their photon rectangles
        if (!k.resident)
            hipLaunchKernelGGL(k_patch_nzbox<double>, dim3((unsigned)k.nb), dim3(64), 0, st, k.d_box, k.d_off, (const double *)k.d_data, k.d_nz);
        jd.nzbox = k.d_nz; jd.nsplit = k.nparts;
        launch_patch_ll<0>(c, im, jd, P * B * k.nparts, st);
    }
}

// step 4: a proposal's value -- a job's parts first, in order (as k_slice_step does), then the bands, in order (the reference's image loop)
static void pll_sum(const std::vector<double> &hout, int64_t P, int B, int nparts, double *ll) {
    for (int64_t p = 0; p < P; p++) {
        double s = 0.0;
        for (int b = 0; b < B; b++) {
            const double *q = hout.data() + (size_t)(p * B + b) * nparts;
            double x = q[0];
            for (int i = 1; i < nparts; i++) x += q[i];
            s += x;
        }
        ll[p] = s;
    }
}

// The resident mode-0 gradient's route, read when a gradient is launched: the photon lists (k_patch_grad_nz.h) iff the option's
// bit is set and the split's lists stand -- a split made under CEL_OPT_PHOTON_LISTS = 2, a direct-form split and a frame of
// 65 536 columns or rows have none, and the dense kernel runs as the value's does.  CEL_OPT_KERNEL is not read.
// `multi`: cel_patch_loglik_multi or the HMC step (cel_patch_loglik's single source keeps the dense kernel).
static bool grad_at_photons(const cel_images *im, bool multi) { return multi && im->ctx->grad_nz && im->split.nz_valid; }

// step 5, the gradient form (k_patch_grad.h): the same records, boxes, offsets, owners and staged data, still in their slots;
// `val` is mode m's value per proposal, slot 0 of its row
static int pll_gradient(cel_images *im, cel_sources *src, const PllCall &k, const std::vector<double> &val, double *ll_out) {
    cel_ctx *c = im->ctx;
    const int B = im->B, mode = k.mode;
    const int64_t P = k.P;
    double *d_sums = nullptr, *d_grad = nullptr;
    const size_t ng = (size_t)P * (7 + B);
    int rc;
    if ((rc = scratch_get(c, SCR_TMP_A, sizeof(double) * GRAD_NS * PGRAD_PARTS * (size_t)(P * B), (void **)&d_sums)) ||
        (rc = scratch_get(c, SCR_TMP_B, sizeof(double) * ng, (void **)&d_grad)))
        return rc;
    int pi = prof_begin(c, CEL_K_PATCH_LL);
    const dim3 grid((unsigned)(P * B * PGRAD_PARTS));
#define PGRAD_LAUNCH(M, TZ, DATA)                                                                                              \
    hipLaunchKernelGGL((k_patch_grad<M, TZ>), grid, dim3(64), 0, c->stream, im->d_bands, B, P, im->d_recs, (const int *)k.d_owner, \
                       (const int4 *)k.d_box, (const int64_t *)k.d_off, (const TZ *)(DATA), (const double *)im->d_nelec, im->H, im->W, d_sums)
    // the resident split's patches: at their photon lists when CEL_OPT_PHOTON_LISTS asks for it (4, 5) and the lists stand
    if (k.i_data && grad_at_photons(im, k.owned))
        hipLaunchKernelGGL(pgrad_nz_sums, grid, dim3(64), 0, c->stream, im->d_bands, B, P, im->d_recs, (const int *)k.d_owner,
                           (const int4 *)k.d_box, (const int64_t *)im->d_nzoff, (const NzEntry *)im->d_nzlist, d_sums);
    else if (k.i_data) PGRAD_LAUNCH(0, int, k.i_data);
    else if (mode == 0) PGRAD_LAUNCH(0, double, k.d_data);
    else if (mode == 1) PGRAD_LAUNCH(1, double, k.d_data);
    else PGRAD_LAUNCH(2, double, k.d_data);
#undef PGRAD_LAUNCH
    hipLaunchKernelGGL(k_patch_grad_chain, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, c->stream, im->d_bands, B, P, im->d_recs,
                       (const int *)k.d_owner, (const int4 *)k.d_box, (const int *)src->d_type, (const double *)src->d_shape,
                       (const double *)src->d_counts, (const double *)d_sums, mode, d_grad);
    std::vector<double> hpe((size_t)(k.exact ? 2 * P : 0));           // the cover flags (pri), then the exact terms
    if (k.exact) {
        // the exact conditional (k_mass_grad.h): the masses and the term per proposal as the exact slice engine forms them, the
        // mass gradient's sums, the same chain rule on them (mode 2: nothing but the sums), and the exact rows from the two
        // (on a masked set under CEL_OPT_SAMPLER_MASK: the observed mass and its derivative, launch for launch)
        launch_proposal_mass(c, im, P, k.d_owner, k.d_mass, P * B);
        hipLaunchKernelGGL(k_sg_exact_terms, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, c->stream, P, B, (const int *)k.d_owner,
                           (const BandDev *)im->d_bands, (const double *)src->d_counts, (const double *)k.d_mass,
                           (const int64_t *)im->d_soff, k.d_exact);
        launch_mass_grad(c, im, P, k.d_owner, k.d_msums);
        hipLaunchKernelGGL(k_patch_grad_chain, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, c->stream, im->d_bands, B, P, im->d_recs,
                           (const int *)k.d_owner, (const int4 *)k.d_box, (const int *)src->d_type, (const double *)src->d_shape,
                           (const double *)src->d_counts, (const double *)k.d_msums, 2, k.d_mg);
        hipLaunchKernelGGL(k_mass_grad_apply, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, c->stream, P, B, (const int *)k.d_owner,
                           (const BandDev *)im->d_bands, (const int64_t *)im->d_soff, (const double *)k.d_mass, (const double *)k.d_mg, d_grad);
        HIP_TRY(hipMemcpyAsync(hpe.data(), k.d_pri, sizeof(double) * P, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(hpe.data() + P, k.d_exact, sizeof(double) * P, hipMemcpyDeviceToHost, c->stream));
    }
    prof_end(c, pi);
    HIP_TRY(hipGetLastError());
    std::vector<double> hg(ng);
    HIP_TRY(hipMemcpyAsync(hg.data(), d_grad, sizeof(double) * ng, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int64_t p = 0; p < P; p++) {
        double v = val[(size_t)p];
        if (k.exact) v = (hpe[(size_t)p] > -INFINITY) ? v + hpe[(size_t)(P + p)] : -INFINITY;     // ll = patch sum; ll += e (uncovered: -inf)
        hg[(size_t)p * (7 + B)] = v;
    }
    memcpy(ll_out, hg.data(), sizeof(double) * ng);
    return CEL_OK;
}

static int pll_run(cel_images *im, cel_sources *src, const int32_t *owner, int64_t NB, const int32_t *boxes, const int64_t *offsets,
                   const double *data, int mem, int mode_arg, double *ll_out, bool multi) {
    PllCall k;
    k.owned = multi;
    int rc = pll_check(im, src, owner, NB, boxes, offsets, data, mode_arg, ll_out, k);
    if (rc || k.P == 0) return rc;
    if ((rc = run_prep(im, src)) || (rc = pll_stage(im, owner, offsets, data, mem, k))) return rc;
    cel_ctx *c = im->ctx;
    if (k.exact)                     // the cover test first: an uncovered proposal's slot retires (its jobs return at their first instructions)
        hipLaunchKernelGGL(k_sg_cover, dim3((unsigned)((k.P + 255) / 256)), dim3(256), 0, c->stream, k.P, im->B, k.d_owner, k.d_pri,
                           (const int4 *)im->d_boxes, (const int *)im->d_status, (const int4 *)im->d_snz);
    const int pi = prof_begin(c, CEL_K_PATCH_LL);
    pll_launch_values(im, k);
    prof_end(c, pi);
    HIP_TRY(hipGetLastError());
    std::vector<double> hout((size_t)(k.P * im->B * k.nparts)), val((size_t)(k.grad ? k.P : 0));
    HIP_TRY(hipMemcpyAsync(hout.data(), k.d_out, sizeof(double) * hout.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // (slot 0 of the gradient form is written once its sums are in)
    pll_sum(hout, k.P, im->B, k.nparts, k.grad ? val.data() : ll_out);
    return k.grad ? pll_gradient(im, src, k, val, ll_out) : CEL_OK;
}

int cel_patch_loglik_multi(cel_images *im, cel_sources *src, const int32_t *owner, int64_t NB,
                           const int32_t *boxes, const int64_t *offsets, const double *data, int mem, int mode_arg,
                           double *ll_out) {
    return pll_run(im, src, owner, NB, boxes, offsets, data, mem, mode_arg, ll_out, true);
}

int cel_patch_loglik(cel_images *im, cel_sources *src, const int32_t *boxes, const int64_t *offsets,
                     const double *data, int mem, int mode, double *ll_out) {
    return pll_run(im, src, nullptr, 1, boxes, offsets, data, mem, mode, ll_out, false);
}

// (Round 4 measured this kernel on a SECOND stream beside the photon split -- its inputs are ready before the split when the
// chain's trace render came last: the split slowed down by 1.35 ms for the 1.7 ms taken off the flux step and the sweep was
// 0.9 ms LONGER than with the two kernels one behind the other; two VALU- and LDS-bound kernels have nothing to give each
// other.  Removed again.)
// may the masses come from the split's own stamp sums (cel_stamp_mass_ready answers it, cel_stamp_mass_begin acts on it)
static bool masses_from_split(const cel_images *im, const cel_sources *src) {
    return !honours_mask(im) && im->ctx->mass_reuse_of() && im->split.sums_of(*src, im->ctx->tail_T) && src->S * im->B <= im->d_massfx.cap;
}

int cel_stamp_mass_ready(cel_images *im, cel_sources *src, int *ready) {
    if (!im || !src || !ready) return fail(CEL_ERR_INVALID, "cel_stamp_mass_ready: null argument");
    *ready = (src->ctx == im->ctx && src->B == im->B && masses_from_split(im, src)) ? 1 : 0;
    return CEL_OK;
}

// the device samplers and the flux step score against the resident split of exactly these sources
static int need_resident_split(const cel_images *im, const cel_sources *src, const char *who, bool sums = false) {
    if (im->split.resident_of(src->S) && (!sums || im->split.ssum_valid)) return CEL_OK;
    return fail(CEL_ERR_INVALID, "%s needs a resident photon split of these %lld sources (have %lld)", who, (long long)src->S,
                (long long)im->split.samp_S);
}

int cel_stamp_mass_begin(cel_images *im, cel_sources *src) {
    if (!im || !src) return fail(CEL_ERR_INVALID, "cel_stamp_mass: null argument");
    if (src->B != im->B || src->ctx != im->ctx) return fail(CEL_ERR_INVALID, "sources do not match images");
    cel_ctx *c = im->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int B = im->B;
    const int64_t S = src->S;
    im->mass.cancel();
    if (S == 0) { im->mass.begin(src->gen, im->split.split_epoch, 0, -1, nullptr, nullptr); return CEL_OK; }
    int rc = CEL_OK;
    // a masked set whose mask is honoured (CEL_OPT_HONOUR_MASK): the unit stamp summed over the UNMASKED pixels of the box -- the
    // split's short cut, which sums every pixel it walks, does not apply (and the masked split leaves it alone)
    const bool observed = honours_mask(im);
    const bool from_split = masses_from_split(im, src);
    if (!from_split || !im->rec.of(*src)) rc = run_prep(im, src);
    if (rc) return rc;
    double *d_out = nullptr;
    if ((rc = scratch_get(c, SCR_VALUES, sizeof(double) * S * B, (void **)&d_out))) return rc;
    int pi = prof_begin(c, CEL_K_MASS);
    if (from_split) {
        // the photon split that has just run on this catalogue (with k_strict_totals before it) summed every unit stamp it
        // evaluated: those sums are the masses; the mass kernel proper runs on the few jobs the short cut does not vouch for
        int *d_ntodo = im->d_mass_todo + im->d_massfx.cap;
        HIP_TRY(hipMemsetAsync(d_ntodo, 0, sizeof(int), c->stream));
        hipLaunchKernelGGL(k_mass_from_fx, dim3((unsigned)((S * B + 255) / 256)), dim3(256), 0, c->stream, S * B, B,
                           (const unsigned long long *)im->d_massfx, (const double *)src->d_counts, (const int *)src->d_type, (const BandDev *)im->d_bands, d_out,
                           im->d_mass_todo, d_ntodo);
        // (how many: read in cel_stamp_mass_end, which launches the mass kernel on exactly those -- none at all in a field
        // without very faint sources; a launch of S B blocks that find nothing to do cost 0.15 ms of the flux step)
        HIP_TRY(hipMemcpyAsync(&c->mail->mass_todo, d_ntodo, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    } else if (observed) {
        hipLaunchKernelGGL(k_stamp_mass_masked, dim3((unsigned)(S * B)), dim3(64), 0, c->stream, im->d_bands, B, im->H, im->W, S,
                           im->d_recs, (const double *)im->d_nelec, c->tail_T, d_out, (const int *)nullptr, (const int *)nullptr);
    } else {
        launch_stamp_mass(c, im, S, nullptr, d_out, S * B);
    }
    prof_end(c, pi);
    HIP_TRY(hipGetLastError());
    im->mass.begin(src->gen, im->split.split_epoch, S * B, from_split ? S : -1, from_split ? im->d_mass_todo.get() : nullptr, d_out);
    return CEL_OK;
}

// the second half of cel_stamp_mass without the copy: the leftovers' kernel queued, im->mass.values complete in stream order; *n_out
// = values (0: nothing pending was there to finish)
static int mass_finish(cel_images *im, int64_t *n_out) {
    if (im->mass.pending < 0) return fail(CEL_ERR_INVALID, "cel_stamp_mass_end without a cel_stamp_mass_begin");
    cel_ctx *c = im->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int64_t n = 0, S_todo = -1;
    im->mass.take(&n, &S_todo);
    *n_out = n;
    if (n == 0) return CEL_OK;
    // A device sampler, a render or a stamp call of another catalogue (or generation) in between re-ran k_prep, and a photon
    // split takes the scratch slot the values wait in: the header allows neither, and what waits is not handed out
    if (!im->mass.intact(im->rec, im->split))
        return fail(CEL_ERR_INVALID, "cel_stamp_mass_end: the source records or the photon split were rebuilt since cel_stamp_mass_begin");
    if (S_todo >= 0) {                  // the short cut's leftovers (cel_stamp_mass_begin)
        HIP_TRY(hipStreamSynchronize(c->stream));
        const int ntodo = c->mail->mass_todo;
        if (ntodo > 0) {
            // Calls that came between _begin and _end (the header lists what may: cel_gamma_streams, cel_samples_fetch,
            // cel_images_set_epsilon) leave the records and the to-do list alone.  Anything that re-ran k_prep for another
            // catalogue, or a photon split that re-allocated its buffers, is caught here instead of scoring stale records:
            if (im->mass.todo_ptr != im->d_mass_todo || !im->mass.intact(im->rec, im->split))
                return fail(CEL_ERR_INVALID, "cel_stamp_mass_end: the source records or the photon split were rebuilt since cel_stamp_mass_begin");
            launch_stamp_mass(c, im, S_todo, nullptr, im->mass.values, ntodo, im->d_mass_todo);
            HIP_TRY(hipGetLastError());
        }
    }
    return CEL_OK;
}

int cel_stamp_mass_end(cel_images *im, double *mass) {
    if (!im || !mass) return fail(CEL_ERR_INVALID, "cel_stamp_mass_end: null argument");
    int64_t n = 0;
    int rc = mass_finish(im, &n);
    if (rc || n == 0) return rc;
    return copy_out(mass, im->mass.values, sizeof(double) * n, CEL_HOST, im->ctx->stream);
}

// Source.resample_fluxes for the whole catalogue on the device (k_flux_step): the stamp masses (cel_stamp_mass's own path, short
// cut and leftovers), the Gamma variates and the new fluxes without a host round trip; the catalogue's expected counts are
// rewritten in place.  One D2H of S * 5 doubles + S ints at the end.
int cel_flux_conditionals(cel_images *im, cel_sources *src, uint64_t seed, double a0, double b0, const int32_t *band_letter,
                          const double *calib, const double *kappa, double *flux_new, int32_t *active) {
    if (!im || !src || !band_letter || !calib || !kappa || !flux_new || !active) return fail(CEL_ERR_INVALID, "cel_flux_conditionals: null argument");
    if (src->B != im->B || src->ctx != im->ctx) return fail(CEL_ERR_INVALID, "sources do not match images");
    { int rm = refuse_masked_unless_honoured(im, "cel_flux_conditionals"); if (rm) return rm; }
    { int rs = need_resident_split(im, src, "cel_flux_conditionals", true); if (rs) return rs; }
    if (!(a0 > 0.0) || !(b0 > 0.0) || !(a0 < 1e300) || !(b0 < 1e300)) return fail(CEL_ERR_INVALID, "cel_flux_conditionals: a0 and b0 must be positive and finite");
    cel_ctx *c = im->ctx;
    const int B = im->B;
    const int64_t S = src->S;
    for (int b = 0; b < B; b++) {
        if (band_letter[b] < 0 || band_letter[b] > 4) return fail(CEL_ERR_INVALID, "cel_flux_conditionals: band letter %d of image %d outside ugriz", band_letter[b], b);
        if (!(calib[b] > 0.0) || !(kappa[b] > 0.0)) return fail(CEL_ERR_INVALID, "cel_flux_conditionals: calib and kappa must be positive");
    }
    HIP_TRY(hipSetDevice(c->device));
    int rc = cel_stamp_mass_begin(im, src);
    if (rc) return rc;
    int64_t n = 0;
    if ((rc = mass_finish(im, &n))) return rc;
    // the per-image constants ride in one small upload: letter[B] | ratio[B] | calib[B] | kappa[B], then the outputs
    char *d = nullptr;
    const int *d_letter = nullptr;
    const double *d_ratio = nullptr;
    double *d_flux = nullptr;
    int *d_act = nullptr;
    auto carve = [&](char *base) {
        Carver k{base};
        d_letter = k.take<int>(MAX_BANDS);
        d_ratio = k.take<double>(3 * MAX_BANDS);        // ratio, calib, kappa
        d_flux = k.take<double>(5 * S);
        d_act = k.take<int>(S);
        return k.off;
    };
    if ((rc = scratch_get(c, SCR_TMP_C, carve(nullptr), (void **)&d))) return rc;
    carve(d);
    struct { int letter[MAX_BANDS]; double ratio[MAX_BANDS], calib[MAX_BANDS], kappa[MAX_BANDS]; } hc;
    memset(&hc, 0, sizeof(hc));
    for (int b = 0; b < B; b++) { hc.letter[b] = band_letter[b]; hc.ratio[b] = kappa[b] / calib[b]; hc.calib[b] = calib[b]; hc.kappa[b] = kappa[b]; }
    static_assert(sizeof(hc) == MAX_BANDS * (sizeof(int) + 3 * sizeof(double)), "packed");
    HIP_TRY(hipMemcpyAsync(d, &hc, sizeof(hc), hipMemcpyHostToDevice, c->stream));      // (pageable: staged before the call returns)
    static_assert(offsetof(decltype(hc), ratio) == sizeof(int) * MAX_BANDS, "the upload is laid out as the block is carved");
    if (S > 0) {
        hipLaunchKernelGGL(k_flux_step, dim3((unsigned)((S * 5 + 255) / 256)), dim3(256), 0, c->stream, S, B, (const double *)im->d_ssum,
                           (const double *)im->mass.values, (const int64_t *)im->d_soff, d_letter, d_ratio, d_ratio + MAX_BANDS, d_ratio + 2 * MAX_BANDS,
                           a0, b0, (unsigned long long)seed, src->d_counts, d_flux, d_act);
        HIP_TRY(hipGetLastError());
        src->all_rows_changed(false);         // the catalogue on the device has new counts
        HIP_TRY(hipMemcpyAsync(flux_new, d_flux, sizeof(double) * 5 * S, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(active, d_act, sizeof(int) * S, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return CEL_OK;
}

// celeste_mcmc.gamma_by_stream on the device (k_gamma_streams): n standard Gamma(a[i]) variates, element i from its own
// streams keyed by (seed, i).  Host arrays in and out.
int cel_gamma_streams(cel_ctx *c, int64_t n, const double *a, uint64_t seed, double *out) {
    if (!c || n < 0 || (n > 0 && (!a || !out))) return fail(CEL_ERR_INVALID, "cel_gamma_streams: bad argument");
    if (n == 0) return CEL_OK;
    for (int64_t i = 0; i < n; i++)
        if (!(a[i] > 0.0) || !(a[i] < 1e300)) return fail(CEL_ERR_INVALID, "cel_gamma_streams: shape parameter %lld is not positive and finite", (long long)i);
    HIP_TRY(hipSetDevice(c->device));
    double *d = nullptr;
    int rc = scratch_get(c, SCR_TMP_C, sizeof(double) * 2 * n, (void **)&d);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d, a, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_gamma_streams, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, (const double *)d,
                       (unsigned long long)seed, d + n);
    HIP_TRY(hipGetLastError());
    return copy_out(out, d + n, sizeof(double) * n, CEL_HOST, c->stream);
}

int cel_stamp_mass(cel_images *im, cel_sources *src, double *mass) {
    if (!mass) return fail(CEL_ERR_INVALID, "cel_stamp_mass: null argument");
    int rc = cel_stamp_mass_begin(im, src);
    return rc ? rc : cel_stamp_mass_end(im, mass);
}

// ---- lock-step slice sampling of the locations, on the device -----------------------------------
// The samplers' conditional log-likelihoods of P proposals against the resident split's patches: the blocks of `dense` score
// their jobs densely (k_patch_ll_hw<0>), those of `nz` at their photons (k_patch_ll_nz; `fuse`: the block that finishes a
// chain's last job steps the chain).  A list names the blocks of a round; `count` is its length where only the device knows
// it (the launch is sized by an upper bound and the kernels stop there).  Every job fills its PLL_PARTS slots of d_ll.
// CEL_OPT_KERNEL = 0 knows no lists: the direct kernel scores every (proposal, band) job in one launch, one slot per job.  -> launches
struct LlBlocks { int64_t n; const int *list, *count; };
static int launch_resident_ll(cel_ctx *c, cel_images *im, int64_t P, const int *d_owner, double *d_ll, bool use_nz,
                              LlBlocks dense, LlBlocks nz, const SliceFuse *fuse) {
    const int B = im->B;
    hipStream_t st = c->stream;
    if (c->variant == 0) {
        int pi = prof_slot(c, CEL_K_PATCH_LL);
        LAUNCH_EV(k_patch_ll<int>, dim3((unsigned)(P * B)), dim3(256), st, EV0(c, pi), EV1(c, pi), im->d_bands, B, P, im->d_recs,
                  d_owner, im->d_sbox, im->d_soff, (const int *)im->d_samp, im->d_nelec, im->H, im->W, 0, d_ll);
        return 1;
    }
    if (dense.n > 0) {
        PatchLlJob<int> j = patch_ll_job(c, im, P, d_owner, d_ll, im->d_sbox, im->d_soff, (const int *)im->d_samp);
        j.nzbox = im->d_snz; j.job_order = dense.list; j.job_count = dense.count; j.nzmode = use_nz ? (const int *)im->d_nzmode : nullptr;
        j.encoded = 1; j.ostride = PLL_PARTS;
        launch_patch_ll<0>(c, im, j, dense.n, st, prof_slot(c, CEL_K_PATCH_LL));
    }
    if (nz.n > 0) {
        int pi = prof_slot(c, CEL_K_PATCH_LL);
        auto go = [&](auto kernel) {
            LAUNCH_EV(kernel, dim3((unsigned)nz.n), dim3(64), st, EV0(c, pi), EV1(c, pi), im->d_bands, B, P, im->d_recs,
                      d_owner, (const int4 *)im->d_sbox, (const int4 *)im->d_snz, (const int *)im->d_nzmode,
                      (const int64_t *)im->d_nzoff, (const NzEntry *)im->d_nzlist, d_ll, nz.list, nz.count, fuse);
        };
        if (fuse) go(k_patch_ll_nz<true>); else go(k_patch_ll_nz<false>);
    }
    return (dense.n > 0) + (nz.n > 0);
}

// The exact conditional's pair (k_slice_gen.h) for the P slots of `prop`: the mass kernel proper, cel_stamp_mass_begin's plain
// branch (its observed branch on a masked set under CEL_OPT_SAMPLER_MASK), on the running chains' jobs
// (a slot that is not scored retires by its owner; a launch of P B blocks that find
// nothing to do costs 0.15 ms, see there), then the term per slot
static void launch_exact_terms(cel_ctx *c, cel_images *im, const cel_sources *prop, int64_t P, const int *d_owner, int64_t n_mass,
                               const int *d_list_mass, double *d_mass, double *d_exact) {
    if (n_mass > 0) launch_proposal_mass(c, im, P, d_owner, d_mass, n_mass, d_list_mass);
    hipLaunchKernelGGL(k_sg_exact_terms, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, c->stream, P, im->B, d_owner, (const BandDev *)im->d_bands,
                       (const double *)prop->d_counts, (const double *)d_mass, (const int64_t *)im->d_soff, d_exact);
}

// a sampler's proposal set of n rows in `own`, built anew with room to spare when the one there is too small
static int ensure_proposals(cel_ctx *c, std::unique_ptr<cel_sources, SourcesDeleter> &own, int64_t n, int B) {
    if (own && own->cap >= n) return CEL_OK;
    own.reset();
    cel_sources *np = nullptr;
    int rc = cel_sources_create(c, n + n / 4 + 16, B, &np);
    if (!rc) own.reset(np);
    return rc;
}

// chains with a negative id are another rank's: they never run here
static int64_t chains_here(const int32_t *chain_ids, int64_t S) {
    return chain_ids ? (int64_t)std::count_if(chain_ids, chain_ids + S, [](int32_t id) { return id >= 0; }) : S;
}

// What the two-slot samplers share -- cel_slice_sample's params 0 / 1, the type move, the HMC step.  Every chain owns the rows
// 2 s and 2 s + 1 of the proposal set im->sgen_prop; a round scores the P = 2 S slots against the resident split.  Here: the facts
// of the call, the scoring arrays (carved from im->d_sgen behind the caller's own state), the upload, the readback of the flag
// words (SliceFlag, k_slice_state.h) into the mailbox's pinned slot and the round's launches.
struct SlotScorer {
    cel_images *const im;
    cel_ctx *const c = im->ctx;
    const hipStream_t st = c->stream;
    const int64_t S, P = 2 * S;
    const int B = im->B;
    const bool exact;                                  // the exact conditional: a cover test, a stamp mass and a term per slot
    const bool mass_list;                              // ... with the running chains' mass jobs listed (otherwise all P B run)
    const bool lists = c->variant != 0;                // block lists; CEL_OPT_KERNEL = 0 scores all P B jobs in one launch
    const bool use_nz = im->split.nz_valid && lists;
    const int ostr = lists ? PLL_PARTS : 1;            // slots per job in d_ll: the recurrence kernels always fill all four
    cel_sources *prop = nullptr;
    double *d_ll = nullptr, *d_mass = nullptr, *d_exact = nullptr;
    int *d_owner = nullptr, *d_ids = nullptr, *d_list = nullptr, *d_list_nz = nullptr, *d_list_mass = nullptr, *d_flags = nullptr;
    int64_t n_dense = P * B, n_nz = 0, n_mass = mass_list ? 0 : P * B;          // the round's blocks and mass jobs, as last read
    int *const h = c->mail->sh.slice_flags;            // the flag words as last read, in the mailbox's pinned slot: h[SF_ERROR], ...

    SlotScorer(cel_images *im_, int64_t S_, bool exact_, bool mass_list_) : im(im_), S(S_), exact(exact_), mass_list(mass_list_) {}

    void take(Carver &k) {
        const size_t n = (size_t)S, nl = lists ? 2 * n * B * PLL_PARTS : 0;
        d_ll = k.take<double>(2 * n * B * ostr);
        d_mass = exact ? k.take<double>(2 * n * B) : nullptr;            // the slots' stamp masses, per (slot, band)
        d_exact = exact ? k.take<double>(2 * n) : nullptr;               // the exact conditional's term per slot (k_sg_exact_terms)
        d_owner = k.take<int>(2 * n);
        d_ids = k.take<int>(n);
        d_list = k.take<int>(nl);                                        // the running chains' blocks: dense, at the photons
        d_list_nz = k.take<int>(nl);
        d_list_mass = mass_list ? k.take<int>(2 * n * B) : nullptr;      // ... and their mass jobs
        d_flags = k.take<int>(SF_WORDS, 16);
    }
    // the proposal set (after the caller has carved im->d_sgen: its own state, then take)
    int proposals() {
        const int rc = ensure_proposals(c, im->sgen_prop, P, B);
        if (!rc) prop = im->sgen_prop.get();
        return rc;
    }
    // the call's directions (or none) and chain ids (or none); the flags cleared
    int upload(double *d_dirs, const double *dirs, int64_t n_doubles, const int32_t *chain_ids) {
        if (dirs) HIP_TRY(hipMemcpyAsync(d_dirs, dirs, sizeof(double) * n_doubles, hipMemcpyHostToDevice, st));
        if (chain_ids) HIP_TRY(hipMemcpyAsync(d_ids, chain_ids, sizeof(int) * S, hipMemcpyHostToDevice, st));
        if (dirs || chain_ids) HIP_TRY(hipStreamSynchronize(st));        // pageable sources must stay valid
        HIP_TRY(hipMemsetAsync(d_flags, 0, sizeof(int) * SF_WORDS, st));
        return CEL_OK;
    }
    // the first `words` flags into h, synchronised; the counts they carry are taken
    int read_counts(int words) {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h, d_flags, sizeof(int) * words, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (lists && words > SF_NZ_BLOCKS) { n_dense = h[SF_DENSE_BLOCKS]; n_nz = h[SF_NZ_BLOCKS]; }
        if (mass_list && words > SF_MASS_JOBS) n_mass = h[SF_MASS_JOBS];
        return CEL_OK;
    }
    // One round on the slots `d_owner` names: their records -- with their own boxes under the exact conditional (cover test, mass),
    // otherwise the patch limits are fixed --, the cover test (its verdict in pri and d_owner), the likelihoods into d_ll, the
    // exact terms into d_exact.  *ll_launches: the likelihood launches
    int score(double *pri, int64_t *ll_launches = nullptr) {
        const int rc = run_prep(im, prop, d_owner, exact ? 0 : 1);
        if (rc) return rc;
        if (exact)
            hipLaunchKernelGGL(k_sg_cover, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, P, B, d_owner, pri, (const int4 *)im->d_boxes,
                               (const int *)im->d_status, (const int4 *)im->d_snz);
        const int n = launch_resident_ll(c, im, P, d_owner, d_ll, use_nz, {n_dense, d_list, nullptr}, {n_nz, d_list_nz, nullptr}, nullptr);
        if (ll_launches) *ll_launches = n;
        if (exact) launch_exact_terms(c, im, prop, P, d_owner, n_mass, d_list_mass, d_mass, d_exact);
        return CEL_OK;
    }
};

// what run_prep(im, src, d_live, nobox) hands k_prep, for the kernels that write a named point's records themselves (k_slice_step,
// SliceFuse); taken after ensure_recs, when the tables stand
static PrepArgs prep_args(const cel_images *im, const cel_sources *src, int nobox) {
    PrepArgs pa;
    pa.bands = im->d_bands; pa.B = im->B; pa.H = im->full_H; pa.W = im->W; pa.win_y0 = im->win_y0; pa.win_h = im->H; pa.S = src->S;
    pa.type = src->d_type; pa.counts = src->d_counts; pa.shape = src->d_shape; pa.rsq_gal = rsq_galaxy();
    pa.recs = im->d_recs; pa.boxes = im->d_boxes; pa.kind = im->d_kind; pa.status = im->d_status; pa.nobox = nobox;
    return pa;
}

int cel_slice_locations(cel_images *im, cel_sources *src, const int32_t *chain_ids, double sigma, uint64_t seed,
                        int max_rounds, double *radec_out, double *llh_out, int64_t *stats) {
    if (!im || !src) return fail(CEL_ERR_INVALID, "cel_slice_locations: null argument");
    { int rm = refuse_masked(im, "cel_slice_locations"); if (rm) return rm; }
    if (src->B != im->B || src->ctx != im->ctx) return fail(CEL_ERR_INVALID, "sources do not match images");
    { int rs = need_resident_split(im, src, "cel_slice_locations"); if (rs) return rs; }
    if (!(sigma > 0.0) || max_rounds < 1) return fail(CEL_ERR_INVALID, "cel_slice_locations: sigma and max_rounds must be positive");
    cel_ctx *c = im->ctx;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int B = im->B;
    const int64_t S = src->S;
    // blocks per (chain, band) job in rounds with at most SLICE_SPLIT_JOBS jobs left (measured at config 3: 4 blocks
    // below 2048 jobs 29.4 ms per location step, below 8192 jobs 29.0; 8 blocks 29.4; without 30.3)
    const int SLICE_SPLIT = PLL_PARTS, SLICE_SPLIT_JOBS = 8192;
    // one allocation, carved (Carver: once for the size, once for the pointers)
    SliceState ss;
    double *d_ll;
    int *d_owner, *d_ids, *d_work, *d_jobs, *d_live, *d_work_nz, *d_jobs_nz, *d_live_nz, *d_tick, *d_need_full, *d_need_live, *d_flags;
    SliceFuse *d_fz;
    auto carve = [&](char *base) {
        Carver k{base};
        const size_t n = (size_t)S, nj = (size_t)S * B * SLICE_SPLIT;
        ss.key = k.take<unsigned long long>(n);
        ss.count = k.take<unsigned long long>(n);
        ss.x = k.take<double>(2 * n);
        ss.x0 = k.take<double>(2 * n);
        ss.lower = k.take<double>(n);
        ss.upper = k.take<double>(n);
        ss.log_u = k.take<double>(n);
        ss.llh_s = k.take<double>(n);
        ss.new_z = k.take<double>(n);
        ss.new_llh = k.take<double>(n);
        d_ll = k.take<double>(nj);
        ss.phase = k.take<int>(n);
        ss.kdir = k.take<int>(n);
        ss.first = k.take<int>(n);
        ss.steps = k.take<int>(n);
        d_owner = k.take<int>(n);
        d_ids = k.take<int>(n);
        // per (job, part) block entries (k_job_work): work estimates, the heaviest-first block lists of a full round, and the
        // running chains' blocks of the late rounds -- for the jobs scored densely and for those scored at their photons
        d_work = k.take<int>(nj);
        d_jobs = k.take<int>(nj);
        d_live = k.take<int>(nj);
        d_work_nz = k.take<int>(nj);
        d_jobs_nz = k.take<int>(nj);
        d_live_nz = k.take<int>(nj);
        // the fused rounds (SliceFuse, k_slice_state.h): per chain its ticket counter and the blocks the full / the live lists hold for it
        d_tick = k.take<int>(n);
        d_need_full = k.take<int>(n);
        d_need_live = k.take<int>(n);
        d_flags = k.take<int>(SFL_WORDS);       // (SliceFlag, k_slice_state.h)
        // the fused rounds' arguments, in device memory: [0] for the full lists, [1] for the live lists (they differ in `need`)
        d_fz = k.take<SliceFuse>(2, 16);
        return k.off;
    };
    HIP_TRY(carved(im->d_slice, st, carve));
    { int rp = ensure_proposals(c, im->slice_prop, S, B); if (rp) return rp; }
    cel_sources *prop = im->slice_prop.get();
    // the proposal set: this catalogue with the locations rewritten every round
    HIP_TRY(hipMemcpyAsync(prop->d_type, src->d_type, sizeof(int) * S, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(prop->d_counts, src->d_counts, sizeof(double) * B * S, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(prop->d_shape, src->d_shape, sizeof(double) * 4 * S, hipMemcpyDeviceToDevice, st));
    prop->S = S;
    if (chain_ids) {
        HIP_TRY(hipMemcpyAsync(d_ids, chain_ids, sizeof(int) * S, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    HIP_TRY(hipMemsetAsync(d_flags, 0, sizeof(int) * SFL_WORDS, st));
    if (c->slice_fuse) HIP_TRY(hipMemsetAsync(d_tick, 0, sizeof(int) * 2 * S, st));    // the tickets and the full lists' block counts
    const unsigned g256 = (unsigned)((S + 255) / 256);
    hipLaunchKernelGGL(k_slice_init, dim3(g256), dim3(256), 0, st, ss, S, src->d_radec, chain_ids ? d_ids : (const int *)nullptr,
                       im->d_soff, B, (unsigned long long)seed, sigma, d_owner);
    // the (chain, band) jobs of a round, heaviest first (the photon rectangles are fixed for the call)
    // The blocks of a round.  With the recurrence kernels every (chain, band) job is one block, or PLL_PARTS blocks when it
    // is long (k_job_work), listed heaviest first; with photon lists a patch is scored either densely (k_patch_ll_hw<0>) or
    // at its photons (k_patch_ll_nz): two lists.  The photon rectangles, lists and routes are fixed for the call.
    const bool use_nz = im->split.nz_valid && c->variant != 0;
    int64_t n_dense = S * B, n_nz = 0;
    if (c->variant != 0) {
        const int nent = (int)(S * B * SLICE_SPLIT);
        hipLaunchKernelGGL(k_job_work, dim3((unsigned)((nent + 255) / 256)), dim3(256), 0, st, src->d_type, im->d_snz, S, B, d_work,
                           (const int *)(use_nz ? im->d_nzmode : nullptr), (const int *)im->d_nnz, use_nz ? d_work_nz : (int *)nullptr,
                           (use_nz && c->slice_fuse) ? d_need_full : (int *)nullptr);
        // members compacted by the whole GPU, then ordered heaviest first by one block (the live-list arrays are free now)
        static_assert(SFL_NZ_JOBS == SFL_DENSE_JOBS + 1, "the two lengths are cleared and read as a pair");
        HIP_TRY(hipMemsetAsync(d_flags + SFL_DENSE_JOBS, 0, sizeof(int) * 2, st));
        hipLaunchKernelGGL(k_list_members, dim3((unsigned)((nent + 255) / 256)), dim3(256), 0, st, d_work, nent, d_live, d_live_nz, d_flags + SFL_DENSE_JOBS);
        hipLaunchKernelGGL(k_order_compact, dim3(1), dim3(1024), 0, st, (const int *)d_live, (const int *)d_live_nz, (const int *)(d_flags + SFL_DENSE_JOBS), d_jobs);
        if (use_nz) {
            hipLaunchKernelGGL(k_list_members, dim3((unsigned)((nent + 255) / 256)), dim3(256), 0, st, d_work_nz, nent, d_live, d_live_nz, d_flags + SFL_NZ_JOBS);
            hipLaunchKernelGGL(k_order_compact, dim3(1), dim3(1024), 0, st, (const int *)d_live, (const int *)d_live_nz, (const int *)(d_flags + SFL_NZ_JOBS), d_jobs_nz);
        }
        int *h_cnt = c->mail->sh.slice_flags;
        h_cnt[1] = 0;
        HIP_TRY(hipMemcpyAsync(h_cnt, d_flags + SFL_DENSE_JOBS, sizeof(int) * (use_nz ? 2 : 1), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        n_dense = h_cnt[0]; n_nz = use_nz ? h_cnt[1] : 0;
    }
    // One launch per round: every patch of the call is scored at its photons (no dense job: the usual case, and config 5's), so
    // the block that finishes a chain's last job of a round steps the chain itself (SliceFuse).  With dense jobs in the call the
    // chains are stepped by k_slice_step as before (the dense kernel carries no ticket).  CEL_OPT_SLICE_FUSE = 0: never fused.
    // MEASURED, AND OFF BY DEFAULT (round 6, kernel traces of ten sweeps per setting, the same chains: the location step's span
    // on the device 12.67 ms unfused; fused in rounds of at most 4 096 blocks 12.65, 12 288: 12.70, 32 768: 12.9, every round:
    // 13.25).  A ticket is a returning atomic every block waits for before it leaves (~2 us of a wave slot) and the stepping block
    // holds its slot ~7 us longer: on a full round (50 000 blocks on 4 096 slots) 45 us more kernel time against the 27 us of the
    // step launch and its two gaps; in the late rounds the step's latency moves from a launch of its own to the end of the
    // likelihood launch and the round gains under 10 us.  c->slice_fuse = N: rounds of at most N blocks are fused (1: every round).
    const bool fuse_ok = use_nz && c->slice_fuse && n_dense == 0 && n_nz > 0;
    bool fused = false;                               // of the batch being queued
    int64_t rounds = 0, evals = 0, queued = 0, live = chains_here(chain_ids, S);
    if (chain_ids && live < 1) live = 1;    // a launch needs a block; k_slice_live_jobs finds nothing to run
    int rc = CEL_OK;
    // The chains advance on the device alone (propose -> records -> likelihoods -> consume), so rounds are queued SLICE_BATCH
    // at a time and the flags read once per batch -- and TWO batches are kept in flight: batch k + 1 is queued before the
    // host waits for batch k's flags, so the queue does not drain while the host takes its turn (with one batch in flight
    // a kernel trace shows the device idle for 50-100 us at every batch boundary; on an idle host the step measures the
    // same either way, 12.6-13.0 ms -- the second batch is there for the hosts that wake up late).
    // A round queued after the last chain has finished scores nothing (every job retires at its first instruction) and
    // is not counted: the price is at most one batch of empty launches at the end.
    const int SLICE_BATCH = 4;                       // (6, 8 and 12 measure the same sweep)
    const int ostr = (c->variant != 0) ? SLICE_SPLIT : 1;        // slots per job in d_ll: the recurrence kernels always fill all four
    // the blocks of a batch: the full heaviest-first lists while (nearly) every chain runs, afterwards the running chains'
    // blocks (k_slice_live_jobs, built behind the batch before).  The host sizes a launch by the newest counts it has READ --
    // those of the batch before the one whose lists the launch walks; chains only retire, so those are upper bounds (times
    // PLL_PARTS where the lists in between began to deal every job), and the kernels stop at the device's own count.
    int64_t live_dense = -1, live_nz = -1;                       // < 0: no live lists read yet
    int *h_flag_slot[2] = {c->mail->sh.slice_flags, c->mail->slice_flags1};
    if ((rc = ensure_recs(im, S * B > 0 ? S * B : 1))) return rc;   // (before the pointers are taken)
    const PrepArgs pa = prep_args(im, prop, 1);                  // what run_prep(im, prop, d_owner, 1) hands k_prep
    SliceFuse fz[2];        // the source of an asynchronous copy: alive until the stream is synchronised at the end of the call
    if (fuse_ok) {
        memset(fz, 0, sizeof(fz));
        for (int k = 0; k < 2; k++) {
            fz[k].tick = d_tick; fz[k].need = k ? d_need_live : d_need_full; fz[k].st = ss; fz[k].ll_pb = d_ll; fz[k].nparts = SLICE_SPLIT;
            fz[k].B = B; fz[k].sigma = sigma; fz[k].flags = d_flags; fz[k].prop_radec = prop->d_radec; fz[k].owner = d_owner; fz[k].pa = pa;
        }
        HIP_TRY(hipMemcpyAsync(d_fz, fz, sizeof(fz), hipMemcpyHostToDevice, st));
    }
    if (!c->slice_ev[0]) {
        HIP_TRY(hipEventCreateWithFlags(&c->slice_ev[0], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&c->slice_ev[1], hipEventDisableTiming));
    }
    int last_par[2] = {0, 0};                                    // parity of a batch's last round: which slot holds its running count
    int deal_of[2] = {0, 0};                                     // whether a batch's live lists dealt every job
    int deal_read = 0;                                           // ... of the batch whose counts live_dense / live_nz are
    int qb = 0, rb = 0;                                          // batches queued / read
    bool finished = false;
    for (;;) {
        while (qb - rb < 2 && queued < max_rounds && !finished) {
            const int nb = (int)std::min<int64_t>(SLICE_BATCH, (int64_t)max_rounds - queued);
            const bool use_live = live_dense >= 0 && (live_dense + live_nz) * 4 < (n_dense + n_nz) * 3;
            // the lists this batch walks are those of batch qb - 1; the counts in hand those of batch rb - 1 <= qb - 1
            const int grow = (use_live && qb >= 1 && deal_of[(qb - 1) & 1] && !deal_read) ? SLICE_SPLIT : 1;
            const int64_t cap_blocks = S * B * SLICE_SPLIT;
            const int64_t gd = use_live ? std::min<int64_t>(live_dense * grow, cap_blocks) : n_dense;
            const int64_t gn = !use_nz ? 0 : (use_live ? std::min<int64_t>(live_nz * grow, cap_blocks) : n_nz);
            fused = fuse_ok && (c->slice_fuse == 1 || gn <= (int64_t)c->slice_fuse);
            for (int k = 0; k < nb; k++) {
                // the first round's points; every later round's were named by the step kernel of the round before
                if (queued == 0) hipLaunchKernelGGL(k_slice_propose, dim3(g256), dim3(256), 0, st, ss, S, prop->d_radec, d_owner, d_flags);
                prop->all_rows_changed(true);
                // the first round's records; every later round's were written by the step kernel that named its points
                if (queued == 0 && (rc = run_prep(im, prop, d_owner, 1))) return rc;      // the patch limits are fixed: no boxes
                launch_resident_ll(c, im, S, d_owner, d_ll, use_nz, {gd, use_live ? d_live : d_jobs, use_live ? d_flags + SF_DENSE_BLOCKS : nullptr},
                                   {gn, use_live ? d_live_nz : d_jobs_nz, use_live ? d_flags + SF_NZ_BLOCKS : nullptr},
                                   fused ? d_fz + (use_live ? 1 : 0) : nullptr);
                if (!fused)
                hipLaunchKernelGGL(k_slice_step, dim3((unsigned)((S + 63) / 64)), dim3(64 * B), 0, st, ss, S, B, ostr, d_ll, sigma, d_flags, (int)queued, prop->d_radec, d_owner,
                                   (k == nb - 1 && c->variant != 0 && !fuse_ok) ? 1 : 0, pa);
                queued++;
            }
            const int slot = qb & 1;
            deal_of[slot] = 0;
            if (c->variant != 0) {          // the running chains' blocks, for the next batch; few chains left: every job dealt
                deal_of[slot] = (live * B <= SLICE_SPLIT_JOBS) ? 1 : 0;
                if (fuse_ok) {                   // (otherwise the batch's last k_slice_step cleared the two counts)
                    static_assert(SFL_LIVE_RUNNING == SF_DENSE_BLOCKS + 2, "the two counts and the running chains are cleared as one");
                    HIP_TRY(hipMemsetAsync(d_flags + SF_DENSE_BLOCKS, 0, sizeof(int) * 3, st));
                    HIP_TRY(hipMemsetAsync(d_need_live, 0, sizeof(int) * S, st));
                }
                hipLaunchKernelGGL(k_slice_live_jobs, dim3((unsigned)((S * B + 255) / 256)), dim3(256), 0, st, ss, S, B, d_live, d_flags + SF_DENSE_BLOCKS,
                                   (const int *)(use_nz ? im->d_nzmode : nullptr), d_live_nz, d_flags + SF_NZ_BLOCKS, (const int *)im->d_nnz,
                                   (const int4 *)im->d_snz, deal_of[slot], fuse_ok ? d_need_live : (int *)nullptr,
                                   fuse_ok ? d_flags + SFL_LIVE_RUNNING : (int *)nullptr);
            }
            HIP_TRY(hipMemcpyAsync(h_flag_slot[slot], d_flags, sizeof(int) * (SFL_RUNNING_ODD + 1), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipEventRecord(c->slice_ev[slot], st));
            HIP_TRY(hipGetLastError());
            last_par[slot] = (int)((queued - 1) & 1);
            qb++;
        }
        if (rb == qb) break;            // nothing in flight: max_rounds reached
        const int slot = rb & 1;
        HIP_TRY(hipEventSynchronize(c->slice_ev[slot]));
        rb++;
        const int *hf = h_flag_slot[slot];
        // the batch's last round's word of the parity pair; a call that may fuse: k_slice_live_jobs' count
        const int running = hf[fuse_ok ? SFL_LIVE_RUNNING : last_par[slot] ? SFL_RUNNING_ODD : SF_RUNNING], err = hf[SF_ERROR];
        live = running;
        if (c->variant != 0) { live_dense = hf[SF_DENSE_BLOCKS]; live_nz = hf[SF_NZ_BLOCKS]; deal_read = deal_of[slot]; }
        if (err & 3) {
            (void)hipStreamSynchronize(st);                      // the batch still in flight works on this call's buffers
            return fail(CEL_ERR_INVALID, (err & 1) ? "Slice sampler got a NaN" : "Slice sampler shrank to zero!");
        }
        if (!fuse_ok) { evals = hf[SF_EVALS]; rounds = hf[SF_ROUNDS]; }
        if (running == 0) finished = true;                       // whatever is still queued scores nothing
        else if (queued >= max_rounds && rb == qb)
            return fail(CEL_ERR_INVALID, "cel_slice_locations: %d rounds without every chain finishing", max_rounds);
        if (finished) break;
    }
    // the new locations replace the catalogue's
    HIP_TRY(hipMemcpyAsync(src->d_radec, ss.x, sizeof(double) * 2 * S, hipMemcpyDeviceToDevice, st));
    src->all_rows_changed(false);
    if (radec_out) HIP_TRY(hipMemcpyAsync(radec_out, ss.x, sizeof(double) * 2 * S, hipMemcpyDeviceToHost, st));
    if (llh_out) HIP_TRY(hipMemcpyAsync(llh_out, ss.new_llh, sizeof(double) * S, hipMemcpyDeviceToHost, st));
    unsigned long long *d_bytes = reinterpret_cast<unsigned long long *>(((uintptr_t)(d_flags + SFL_BYTES) + 7) & ~(uintptr_t)7);
    if (stats) {
        // algorithmic bytes of the call: a chain made 1 + steps[s] evaluations (the first direction's level, then one
        // per shrink step), each walking its photon rectangles
        HIP_TRY(hipMemsetAsync(d_bytes, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(k_slice_bytes, dim3(g256), dim3(256), 0, st, ss, S, B, (const int4 *)im->d_snz, d_bytes,
                           (const int *)(use_nz ? im->d_nzmode : nullptr), (const int64_t *)im->d_nzoff, fuse_ok ? d_flags + SFL_EVALS_END : (int *)nullptr);
        HIP_TRY(hipMemcpyAsync(&c->mail->sh.w.slice_bytes, d_bytes, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        if (fuse_ok) HIP_TRY(hipMemcpyAsync(h_flag_slot[1], d_flags + SFL_EVALS_END, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (stats) {
        if (fuse_ok) { evals = h_flag_slot[1][0]; rounds = h_flag_slot[1][1]; }    // what the per-round counts of the unfused rounds add up to
        stats[0] = rounds; stats[1] = evals;
        stats[2] = (int64_t)c->mail->sh.w.slice_bytes;
        stats[3] = queued;
    }
    return CEL_OK;
}

// The star <-> galaxy move (k_type_move.h): cel_slice_sample's param 2, after its refusals.  One Metropolis-Hastings proposal
// per chain against the resident split, both slots of every running chain scored in one round of the slice samplers' launches.
static int slice_type_move(cel_images *im, cel_sources *src, const int32_t *chain_ids, const double *dirs, int numdir,
                           uint64_t seed, double *x_out, double *llh_out, int64_t *stats) {
    if (!dirs || numdir != 1)
        return fail(CEL_ERR_INVALID, "cel_slice_sample: the type move (param 2) needs dirs = S rows of (theta, sigma, phi, rho, h) and numdir = 1");
    cel_ctx *c = im->ctx;
    const int B = im->B;
    const int64_t S = src->S;
    for (int64_t s = 0; s < S; s++)
        if (!(chain_ids && chain_ids[s] < 0) && !std::isfinite(dirs[5 * s + 4]))
            return fail(CEL_ERR_INVALID, "cel_slice_sample: the type move's h of chain %lld is not finite", (long long)s);
    const bool exact = c->slice_conditional == 1;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    SlotScorer sc(im, S, exact, exact);
    // one allocation, carved: the move's own state, then the scorer's arrays
    TypeMove tm;
    double *d_dirs, *d_out;
    int *d_flag;
    auto carve = [&](char *base) {
        Carver k{base};
        const size_t n = (size_t)S;
        tm.log_u = k.take<double>(n);
        tm.h = k.take<double>(n);
        tm.pri = k.take<double>(2 * n);
        d_dirs = k.take<double>(5 * n);
        d_out = k.take<double>(6 * n);                        // the new type and shape per chain, then log alpha per chain
        d_flag = k.take<int>(n);                              // right behind d_out: one readback takes both
        tm.run = k.take<int>(n);
        sc.take(k);
        return k.off;
    };
    HIP_TRY(carved(im->d_sgen, st, carve));
    int rc = sc.proposals();
    if (rc) return rc;
    cel_sources *prop = sc.prop;
    const int64_t P = sc.P;
    const bool lists = sc.lists;
    int *const d_owner = sc.d_owner, *const d_flags = sc.d_flags;
    if (S == 0) {
        if (stats) { stats[0] = 1; stats[1] = 0; stats[2] = 0; stats[3] = 0; }
        return CEL_OK;
    }
    if ((rc = sc.upload(d_dirs, dirs, 5 * S, chain_ids))) return rc;
    const unsigned g256 = (unsigned)((S + 255) / 256), p256 = (unsigned)((P + 255) / 256), j256 = (unsigned)((S * B + 255) / 256);
    hipLaunchKernelGGL(k_tm_fill, dim3(p256), dim3(256), 0, st, tm, S, B, (const int *)src->d_type, (const double *)src->d_radec,
                       (const double *)src->d_counts, (const double *)src->d_shape, (const double *)d_dirs,
                       chain_ids ? (const int *)sc.d_ids : (const int *)nullptr, (const int64_t *)im->d_soff, (unsigned long long)seed,
                       prop->d_type, prop->d_radec, prop->d_counts, prop->d_shape, d_owner);
    prop->S = P;
    prop->all_rows_changed(true);
    if (lists || exact) {
        const int64_t live = chains_here(chain_ids, S);
        hipLaunchKernelGGL(k_tm_jobs, dim3(j256), dim3(256), 0, st, tm, S, B, (const int *)(sc.use_nz ? im->d_nzmode : nullptr),
                           (const int *)im->d_nnz, (const int4 *)im->d_snz, (live * 2 * B <= 8192) ? 1 : 0,
                           lists ? sc.d_list : (int *)nullptr, d_flags + SF_DENSE_BLOCKS, sc.d_list_nz, d_flags + SF_NZ_BLOCKS,
                           sc.d_list_mass, d_flags + SF_MASS_JOBS);
        if ((rc = sc.read_counts(SF_MASS_JOBS + 1))) return rc;
    }
    int64_t launches = 0;
    if ((rc = sc.score(tm.pri, &launches))) return rc;
    hipLaunchKernelGGL(k_tm_decide, dim3(g256), dim3(256), 0, st, tm, S, B, sc.ostr, (const double *)sc.d_ll, (const double *)sc.d_exact,
                       (const double *)prop->d_shape, (int *)src->d_type, (double *)src->d_shape, d_out, d_flag, d_flags + SF_ERROR);
    HIP_TRY(hipGetLastError());
    src->all_rows_changed(true);          // the catalogue on the device has new rows, types among them
    // one readback: the rows, log alpha and the flags lie one behind the other (the flags behind 6 S doubles)
    static_assert(sizeof(double) == 2 * sizeof(int), "the readback's layout");
    std::vector<double> back((size_t)(6 * S + (S + 1) / 2));
    const size_t back_bytes = sizeof(double) * 6 * S + sizeof(int) * S;
    HIP_TRY(hipMemcpyAsync(back.data(), d_out, back_bytes, hipMemcpyDeviceToHost, st));
    if ((rc = sc.read_counts(SF_ERROR + 1))) return rc;       // (synchronises: `back` is complete)
    const int *hf = reinterpret_cast<const int *>(back.data() + 6 * S);
    int64_t running = 0, accepted = 0;
    std::vector<int32_t> types((size_t)S);
    for (int64_t s = 0; s < S; s++) {
        types[(size_t)s] = (int32_t)back[(size_t)(5 * s)];
        running += hf[s] >= 0;
        accepted += hf[s] == 1;
    }
    src->types_known(types.data(), S);
    if (x_out) memcpy(x_out, back.data(), sizeof(double) * 5 * S);
    if (llh_out) memcpy(llh_out, back.data() + 5 * S, sizeof(double) * S);
    if (stats) { stats[0] = 1; stats[1] = 2 * running; stats[2] = accepted; stats[3] = launches; }
    if (sc.h[SF_ERROR] & 1)
        return fail(CEL_ERR_INVALID, "cel_slice_sample: the type move found a state outside its own conditional (its current row scores -inf)");
    return CEL_OK;
}

// The HMC step (k_hmc.h): cel_slice_sample's param 3, after its refusals.  Every running chain's trajectory is queued on the
// stream -- per leapfrog step the gradient form's two launches on the proposal set (one slot per chain) and one k_hmc_step --,
// then q0 and qL are scored as the type move scores its two slots; one synchronisation for the job counts, one readback.
static int slice_hmc(cel_images *im, cel_sources *src, const int32_t *chain_ids, const double *dirs, int numdir, double eps,
                     double phi_max, uint64_t seed, int L, double *x_out, double *llh_out, int64_t *stats) {
    if (!dirs || numdir != 2 * HMC_D)
        return fail(CEL_ERR_INVALID, "cel_slice_sample: the HMC step (param 3) needs dirs = S rows of (momentum[6], inverse mass[6]) and numdir = 12");
    cel_ctx *c = im->ctx;
    // CEL_OPT_GRAD_CONDITIONAL = 1: v and g are the exact conditional's (k_mass_grad.h); CEL_OPT_SLICE_CONDITIONAL is not read then
    const bool exact = c->grad_conditional == 1;
    if (!exact && c->slice_conditional == 1)
        return fail(CEL_ERR_INVALID, "cel_slice_sample: the HMC step (param 3): the exact conditional's stamp-mass term has no analytic derivative yet "
                                     "(CEL_OPT_SLICE_CONDITIONAL = 0 only); the exact HMC step is CEL_OPT_GRAD_CONDITIONAL = 1");
    if (im->win_y0 != 0 || im->full_H != im->H)
        return fail(CEL_ERR_INVALID, "cel_slice_sample: the HMC step (param 3) is not supported on an image set with a row window "
                                     "(cel_images_set_window): the gradient form refuses it");
    if (L > 1024) return fail(CEL_ERR_INVALID, "cel_slice_sample: the HMC step (param 3) takes 1 <= max_rounds <= 1024 leapfrog steps");
    if (!std::isfinite(eps)) return fail(CEL_ERR_INVALID, "cel_slice_sample: the HMC step's eps (sigma) must be finite");
    const int B = im->B;
    const int64_t S = src->S;
    // a running chain's momentum and inverse mass (the entries it reads: a star's are 0, 1; where the host does not know the
    // types, all six)
    const bool types = (int64_t)src->h_type.size() == S;
    for (int64_t s = 0; s < S; s++) {
        if (chain_ids && chain_ids[s] < 0) continue;
        const int t = types ? src->h_type[(size_t)s] : 1;
        if (t != 0 && t != 1) continue;
        for (int i = 0; i < (t == 1 ? HMC_D : 2); i++) {
            const double p0 = dirs[2 * HMC_D * s + i], m = dirs[2 * HMC_D * s + HMC_D + i];
            if (!std::isfinite(p0)) return fail(CEL_ERR_INVALID, "cel_slice_sample: the HMC step's momentum %d of chain %lld is not finite", i, (long long)s);
            if (!std::isfinite(m) || m < 0.0)
                return fail(CEL_ERR_INVALID, "cel_slice_sample: the HMC step's inverse mass %d of chain %lld is negative or not finite", i, (long long)s);
        }
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    SlotScorer sc(im, S, exact, false);                       // q0 / qL are scored with every mass job: no list
    // one allocation, carved: the step's own state, then the scorer's arrays
    Hmc hm;
    double *d_dirs, *d_sums, *d_grad, *d_out, *d_msums = nullptr, *d_mg = nullptr, *d_cpri = nullptr;
    int *d_owner, *d_flag;
    auto carve = [&](char *base) {
        Carver k{base};
        const size_t n = (size_t)S;
        hm.q = k.take<double>(HMC_D * n);
        hm.p = k.take<double>(HMC_D * n);
        hm.p0 = k.take<double>(HMC_D * n);
        hm.im = k.take<double>(HMC_D * n);
        hm.log_u = k.take<double>(n);
        hm.k0 = k.take<double>(n);
        hm.pri = k.take<double>(2 * n);
        d_dirs = k.take<double>(2 * HMC_D * n);
        d_sums = k.take<double>((size_t)GRAD_NS * PGRAD_PARTS * n * B);      // k_patch_grad's sums per (chain, band, part)
        d_grad = k.take<double>(n * (7 + B));                                // the mode-8 rows
        d_out = k.take<double>((2 * HMC_D + 1) * n);          // q and the momentum per chain, then log alpha per chain
        d_flag = k.take<int>(n);                              // right behind d_out, and the evaluations behind it: one readback
        hm.nev = k.take<int>(n);
        hm.run = k.take<int>(n);
        hm.dead = k.take<int>(n);
        d_owner = k.take<int>(n);                             // of the trajectory's one slot per chain
        sc.take(k);                                           // (its sc.d_owner: of the two scored slots)
        if (exact) {
            d_msums = k.take<double>((size_t)GRAD_NS * PGRAD_PARTS * n * B);     // k_mass_grad's sums per (chain, band, part)
            d_mg = k.take<double>(n * (7 + B));               // the chain rule on them
            d_cpri = k.take<double>(n);                       // k_sg_cover's flag per gradient evaluation (owner carries the verdict)
        }
        return k.off;
    };
    HIP_TRY(carved(im->d_sgen, st, carve));
    int rc = sc.proposals();
    if (rc) return rc;
    cel_sources *prop = sc.prop;
    const int64_t P = sc.P;
    double *const d_mass = sc.d_mass;
    int *const d_flags = sc.d_flags;
    if (S == 0) {
        if (stats) { stats[0] = L; stats[1] = 0; stats[2] = 0; stats[3] = 0; }
        return CEL_OK;
    }
    rc = ensure_recs(im, P * B);                              // (the records of both proposal sets: nothing grows between the launches)
    if (rc || (rc = sc.upload(d_dirs, dirs, 2 * HMC_D * S, chain_ids))) return rc;
    if (exact) HIP_TRY(hipMemsetAsync(sc.d_exact, 0, sizeof(double) * 2 * S, st));   // (a slot that is not scored gets no term)
    const unsigned g256 = (unsigned)((S + 255) / 256), j256 = (unsigned)((S * B + 255) / 256);
    hipLaunchKernelGGL(k_hmc_fill, dim3(g256), dim3(256), 0, st, hm, S, B, phi_max, (const int *)src->d_type, (const double *)src->d_radec,
                       (const double *)src->d_counts, (const double *)src->d_shape, (const double *)d_dirs,
                       chain_ids ? (const int *)sc.d_ids : (const int *)nullptr, (const int64_t *)im->d_soff, (unsigned long long)seed,
                       prop->d_type, prop->d_radec, prop->d_counts, prop->d_shape, d_owner, d_flags + SF_ERROR);
    int64_t launches = 1;
    if (sc.lists) {                                            // the two slots' blocks of every running chain (k_tm_jobs on this step's `run`)
        TypeMove view{nullptr, nullptr, nullptr, hm.run};
        const int64_t live = chains_here(chain_ids, S);
        hipLaunchKernelGGL(k_tm_jobs, dim3(j256), dim3(256), 0, st, view, S, B, (const int *)(sc.use_nz ? im->d_nzmode : nullptr),
                           (const int *)im->d_nnz, (const int4 *)im->d_snz, (live * 2 * B <= 8192) ? 1 : 0, sc.d_list, d_flags + SF_DENSE_BLOCKS,
                           sc.d_list_nz, d_flags + SF_NZ_BLOCKS, (int *)nullptr, (int *)nullptr);
        if ((rc = sc.read_counts(SF_NZ_BLOCKS + 1))) return rc;
        launches++;
    }
    // L + 1 gradients, a step behind each but the last: nothing here depends on what the device finds
    // (their route -- the dense patches or the photon lists -- is chosen once for the call: grad_at_photons)
    const bool grad_nz = grad_at_photons(im, true);
    for (int l = 0; l <= L; l++) {
        prop->S = S;
        prop->all_rows_changed(true);
        // the patch limits are fixed: no boxes -- but the exact conditional needs the proposals' own (cover test, mass)
        if ((rc = run_prep(im, prop, d_owner, exact ? 0 : 1))) return rc;
        if (exact) {
            hipLaunchKernelGGL(k_sg_cover, dim3(g256), dim3(256), 0, st, S, B, d_owner, d_cpri, (const int4 *)im->d_boxes,
                               (const int *)im->d_status, (const int4 *)im->d_snz);
            hipLaunchKernelGGL(k_hmc_cover, dim3(g256), dim3(256), 0, st, hm, S, (const int *)d_owner, l == 0 ? 1 : 0);
            launches += 2;
        }
        const int pi = prof_begin(c, CEL_K_PATCH_LL);
        if (grad_nz)
            hipLaunchKernelGGL(pgrad_nz_sums, dim3((unsigned)(S * B * PGRAD_PARTS)), dim3(64), 0, st, im->d_bands, B, S, im->d_recs,
                               (const int *)d_owner, (const int4 *)im->d_sbox, (const int64_t *)im->d_nzoff,
                               (const NzEntry *)im->d_nzlist, d_sums);
        else
            hipLaunchKernelGGL((k_patch_grad<0, int>), dim3((unsigned)(S * B * PGRAD_PARTS)), dim3(64), 0, st, im->d_bands, B, S, im->d_recs,
                               (const int *)d_owner, (const int4 *)im->d_sbox, (const int64_t *)im->d_soff, (const int *)im->d_samp,
                               (const double *)im->d_nelec, im->H, im->W, d_sums);
        hipLaunchKernelGGL(k_patch_grad_chain, dim3(g256), dim3(256), 0, st, im->d_bands, B, S, im->d_recs, (const int *)d_owner,
                           (const int4 *)im->d_sbox, (const int *)prop->d_type, (const double *)prop->d_shape,
                           (const double *)prop->d_counts, (const double *)d_sums, 0, d_grad);
        if (exact) {                 // the mass, its gradient's sums, the chain rule on them, the exact rows
            launch_proposal_mass(c, im, S, d_owner, d_mass, S * B);
            launch_mass_grad(c, im, S, d_owner, d_msums);
            hipLaunchKernelGGL(k_patch_grad_chain, dim3(g256), dim3(256), 0, st, im->d_bands, B, S, im->d_recs, (const int *)d_owner,
                               (const int4 *)im->d_sbox, (const int *)prop->d_type, (const double *)prop->d_shape,
                               (const double *)prop->d_counts, (const double *)d_msums, 2, d_mg);
            hipLaunchKernelGGL(k_mass_grad_apply, dim3(g256), dim3(256), 0, st, S, B, (const int *)d_owner, (const BandDev *)im->d_bands,
                               (const int64_t *)im->d_soff, (const double *)d_mass, (const double *)d_mg, d_grad);
            launches += 4;
        }
        prof_end(c, pi);
        launches += 3;
        if (l < L) {
            hipLaunchKernelGGL(k_hmc_step, dim3(g256), dim3(256), 0, st, hm, S, B, l == 0 ? 1 : 0, eps, phi_max, (const int *)src->d_type,
                               (const double *)d_grad, prop->d_radec, prop->d_shape, d_owner);
            launches++;
        }
    }
    hipLaunchKernelGGL(k_hmc_slots, dim3(g256), dim3(256), 0, st, hm, S, B, eps, phi_max, (const int *)src->d_type, (const double *)src->d_radec,
                       (const double *)src->d_counts, (const double *)src->d_shape, (const double *)d_grad, prop->d_type, prop->d_radec,
                       prop->d_counts, prop->d_shape, sc.d_owner);
    prop->S = P;
    prop->all_rows_changed(true);
    int64_t ll_launches = 0;         // the two scored slots: records; exact: their cover test, every mass job and the terms
    if ((rc = sc.score(hm.pri, &ll_launches))) return rc;
    launches += 2 + ll_launches + (exact ? 3 : 0);            // (k_hmc_slots and k_prep; k_sg_cover, the mass kernel, k_sg_exact_terms)
    hipLaunchKernelGGL(k_hmc_decide, dim3(g256), dim3(256), 0, st, hm, S, B, sc.ostr, (const double *)sc.d_ll, (const double *)sc.d_exact,
                       (const int *)src->d_type, (double *)src->d_radec, (double *)src->d_shape, d_out, d_flag, d_flags + SF_ERROR);
    launches++;
    HIP_TRY(hipGetLastError());
    src->all_rows_changed(false);         // the catalogue on the device has new locations and shapes; the types stand
    // one readback: the rows, log alpha, the flags and the evaluations lie one behind the other
    static_assert(sizeof(double) == 2 * sizeof(int), "the readback's layout");
    const int64_t nd = (2 * HMC_D + 1) * S;
    std::vector<double> back((size_t)(nd + S));
    HIP_TRY(hipMemcpyAsync(back.data(), d_out, sizeof(double) * nd + sizeof(int) * 2 * S, hipMemcpyDeviceToHost, st));
    if ((rc = sc.read_counts(SF_ERROR + 1))) return rc;       // (synchronises: `back` is complete)
    const int *hf = reinterpret_cast<const int *>(back.data() + nd), *hn = hf + S;
    int64_t evals = 0, accepted = 0;
    for (int64_t s = 0; s < S; s++) {
        evals += hn[s];
        accepted += hf[s] == 1;
    }
    if (x_out) memcpy(x_out, back.data(), sizeof(double) * 2 * HMC_D * S);
    if (llh_out) memcpy(llh_out, back.data() + 2 * HMC_D * S, sizeof(double) * S);
    if (stats) { stats[0] = L; stats[1] = evals; stats[2] = accepted; stats[3] = launches; }
    if (sc.h[SF_ERROR] & 1)
        return fail(CEL_ERR_INVALID, "cel_slice_sample: the HMC step found a state outside its own conditional (its current row scores -inf)");
    return CEL_OK;
}

// The general slice sampler (k_slice_gen.h): random directions, stepping out by doubling, D = 2 or 4.
static int samples_moments(cel_images *im, const cel_sources *src, int64_t *mom);      // (below, with the split)
int cel_slice_sample(cel_images *im, cel_sources *src, int param, const int32_t *chain_ids, const double *dirs, int numdir,
                     int step_out, int max_steps_out, double sigma, double phi_max, uint64_t seed, int max_rounds,
                     double *x_out, double *llh_out, int64_t *stats) {
    // param CEL_SLICE_MOMENTS: no sampler -- the moments of the resident split into stats (any set that holds a split; src may be null)
    if (im && param == CEL_SLICE_MOMENTS) return samples_moments(im, src, stats);
    if (!im || !src) return fail(CEL_ERR_INVALID, "cel_slice_sample: null argument");
    // (a masked set: refused, unless CEL_OPT_SAMPLER_MASK and CEL_OPT_HONOUR_MASK hold and this call runs the exact conditional)
    { int rm = refuse_masked_sampler(im, "cel_slice_sample", param == 3 ? im->ctx->grad_conditional == 1 : im->ctx->slice_conditional == 1);
      if (rm) return rm; }
    // CEL_OPT_SLICE_CONDITIONAL = 1: the exact conditional (k_slice_gen.h) -- the proposal's stamp mass on its own box and the
    // cover test per round
    const bool exact = im->ctx->slice_conditional == 1;
    if (exact && (im->win_y0 != 0 || im->full_H != im->H))
        return fail(CEL_ERR_INVALID, "cel_slice_sample: the exact conditional (CEL_OPT_SLICE_CONDITIONAL) is not supported on an image set "
                                     "with a row window (cel_images_set_window): its cover test is not window-relative");
    if (src->B != im->B || src->ctx != im->ctx) return fail(CEL_ERR_INVALID, "sources do not match images");
    { int rs = need_resident_split(im, src, "cel_slice_sample"); if (rs) return rs; }
    if (param < 0 || param > 3) return fail(CEL_ERR_INVALID, "cel_slice_sample: param must be 0 (location), 1 (shape), 2 (type), 3 (HMC) or 10 (the split's moments)");
    if (!(sigma > 0.0) || max_rounds < 1 || max_steps_out < 0) return fail(CEL_ERR_INVALID, "cel_slice_sample: sigma and max_rounds must be positive");
    if (param == 2) return slice_type_move(im, src, chain_ids, dirs, numdir, seed, x_out, llh_out, stats);
    if (param == 3) return slice_hmc(im, src, chain_ids, dirs, numdir, sigma, phi_max, seed, max_rounds, x_out, llh_out, stats);
    const int D = param ? 4 : 2;
    const int compwise = dirs ? 0 : 1;
    const int ndir = compwise ? D : numdir;
    if (ndir < 1 || ndir > 64) return fail(CEL_ERR_INVALID, "cel_slice_sample: numdir must be in [1, 64]");
    cel_ctx *c = im->ctx;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int B = im->B;
    const int64_t S = src->S;
    SlotScorer sc(im, S, exact, exact);
    // one allocation, carved: the sampler's own state, then the scorer's arrays
    SliceGen g;
    SliceState rs;
    double *d_dirs;
    auto carve = [&](char *base) {
        Carver k{base};
        const size_t n = (size_t)S;
        rs.key = k.take<unsigned long long>(n);
        rs.count = k.take<unsigned long long>(n);
        g.key = rs.key; g.count = rs.count;
        g.x = k.take<double>(n * D);
        g.x0 = k.take<double>(n * D);
        g.dir = k.take<double>(n * D);
        g.lower = k.take<double>(n);
        g.upper = k.take<double>(n);
        g.log_u = k.take<double>(n);
        g.llh_s = k.take<double>(n);
        g.new_z = k.take<double>(n);
        g.new_llh = k.take<double>(n);
        g.start_lower = k.take<double>(n);
        g.start_upper = k.take<double>(n);
        g.acc_L = k.take<double>(n);
        g.acc_U = k.take<double>(n);
        g.pri = k.take<double>(2 * n);
        d_dirs = k.take<double>(n * ndir * D);
        g.phase = k.take<int>(n);
        g.kdir = k.take<int>(n);
        g.l_out = k.take<int>(n);
        g.u_out = k.take<int>(n);
        g.order = k.take<int>(n * D);
        sc.take(k);
        return k.off;
    };
    HIP_TRY(carved(im->d_sgen, st, carve));
    int rc = sc.proposals();
    if (rc) return rc;
    cel_sources *prop = sc.prop;
    int *const d_owner = sc.d_owner, *const d_flags = sc.d_flags;
    g.D = D; g.ndir = ndir; g.compwise = compwise; g.step_out = step_out ? 1 : 0; g.max_steps_out = max_steps_out; g.param = param;
    g.sigma = sigma; g.phi_max = param ? phi_max : 0.0; g.dirs = compwise ? nullptr : d_dirs;
    if ((rc = sc.upload(d_dirs, dirs, S * ndir * D, chain_ids))) return rc;      // (compwise: no dirs)
    const unsigned g256 = (unsigned)((S + 255) / 256);
    // the proposal set: every chain's source twice, the sampled parameter rewritten every round
    hipLaunchKernelGGL(k_sg_fill, dim3((unsigned)((2 * S + 255) / 256)), dim3(256), 0, st, S, B, (const int *)src->d_type,
                       (const double *)src->d_radec, (const double *)src->d_counts, (const double *)src->d_shape,
                       prop->d_type, prop->d_radec, prop->d_counts, prop->d_shape);
    prop->S = 2 * S;
    hipLaunchKernelGGL(k_sg_init, dim3(g256), dim3(256), 0, st, g, rs, S, (const double *)(param ? src->d_shape : src->d_radec),
                       chain_ids ? (const int *)sc.d_ids : (const int *)nullptr, (const int64_t *)im->d_soff, B, (const int *)src->d_type,
                       (unsigned long long)seed);
    int64_t rounds = 0, evals = 0, queued = 0;
    const int BATCH = 4;
    const int64_t DEAL_ALL_BELOW = 8192;          // (chain, slot, band) jobs: fewer than the GPU has wave slots for -- deal every job
    int64_t live = S;                             // chains running at the last readback
    const int nflags = (exact ? SF_MASS_JOBS : SF_NZ_BLOCKS) + 1;
    // the running chains' blocks and mass jobs: the first batch's now (their counts come back at once), every later batch's behind
    // the batch before it (the flags were cleared by the upload, then by `again`)
    auto list_jobs = [&](bool again, int deal_all) {
        const unsigned j256 = (unsigned)((S * B + 255) / 256);
        if (sc.lists) {
            if (again) HIP_TRY(hipMemsetAsync(d_flags + SF_DENSE_BLOCKS, 0, sizeof(int) * 2, st));
            hipLaunchKernelGGL(k_sg_live_jobs, dim3(j256), dim3(256), 0, st, g, S, B, (const int *)(sc.use_nz ? im->d_nzmode : nullptr),
                               (const int *)im->d_nnz, (const int4 *)im->d_snz, deal_all, sc.d_list, d_flags + SF_DENSE_BLOCKS, sc.d_list_nz,
                               d_flags + SF_NZ_BLOCKS);
        }
        if (exact) {
            if (again) HIP_TRY(hipMemsetAsync(d_flags + SF_MASS_JOBS, 0, sizeof(int), st));
            hipLaunchKernelGGL(k_sg_mass_jobs, dim3(j256), dim3(256), 0, st, g, S, B, sc.d_list_mass, d_flags + SF_MASS_JOBS);
        }
        return (int)CEL_OK;
    };
    if ((rc = list_jobs(false, 0))) return rc;
    if ((sc.lists || exact) && (rc = sc.read_counts(nflags))) return rc;
    for (;;) {
        const int nb = (int)std::min<int64_t>(BATCH, (int64_t)max_rounds - queued);
        for (int k = 0; k < nb; k++) {
            hipLaunchKernelGGL(k_sg_propose, dim3(g256), dim3(256), 0, st, g, rs, S, param ? prop->d_shape : prop->d_radec, d_owner, d_flags,
                               queued == 0 ? 1 : 0);
            prop->all_rows_changed(true);
            if ((rc = sc.score(g.pri))) return rc;
            if (exact)
                hipLaunchKernelGGL(k_sg_consume_exact, dim3(g256), dim3(256), 0, st, g, rs, S, B, sc.ostr, (const double *)sc.d_ll, d_flags,
                                   (const double *)sc.d_exact);
            else
                hipLaunchKernelGGL(k_sg_consume, dim3(g256), dim3(256), 0, st, g, rs, S, B, sc.ostr, (const double *)sc.d_ll, d_flags);
            queued++;
        }
        // the next batch's blocks: the chains still running now
        if ((rc = list_jobs(true, (live * 2 * B <= DEAL_ALL_BELOW) ? 1 : 0)) || (rc = sc.read_counts(nflags))) return rc;
        const int running = sc.h[SF_RUNNING], err = sc.h[SF_ERROR];
        live = running;
        if (err & 1) return fail(CEL_ERR_INVALID, "Slice sampler got a NaN");
        if (err & 2) return fail(CEL_ERR_INVALID, "Slice sampler shrank to zero!");
        evals = sc.h[SF_EVALS];
        rounds = sc.h[SF_ROUNDS];
        if (running == 0) break;
        if (queued >= max_rounds) return fail(CEL_ERR_INVALID, "cel_slice_sample: %d rounds without every chain finishing", max_rounds);
    }
    // the new states replace the catalogue's
    HIP_TRY(hipMemcpyAsync(param ? src->d_shape : src->d_radec, g.x, sizeof(double) * D * S, hipMemcpyDeviceToDevice, st));
    src->all_rows_changed(false);
    if (x_out) HIP_TRY(hipMemcpyAsync(x_out, g.x, sizeof(double) * D * S, hipMemcpyDeviceToHost, st));
    if (llh_out) HIP_TRY(hipMemcpyAsync(llh_out, g.new_llh, sizeof(double) * S, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (stats) { stats[0] = rounds; stats[1] = evals; stats[2] = 0; stats[3] = queued; }
    return CEL_OK;
}

// ---- photon split -------------------------------------------------------------------------------
int cel_source_boxes(cel_images *im, cel_sources *src, int32_t *boxes, int32_t *status) {
    if (!im || !src || !boxes || !status) return fail(CEL_ERR_INVALID, "cel_source_boxes: null argument");
    if (src->B != im->B || src->ctx != im->ctx) return fail(CEL_ERR_INVALID, "sources do not match images");
    cel_ctx *c = im->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc = host_boxes(im, src);
    if (rc) return rc;
    const int64_t n = src->S * im->B;
    for (int64_t i = 0; i < n; i++) {
        const int4 b = im->h_boxes[(size_t)i];
        boxes[4 * i + 0] = b.z; boxes[4 * i + 1] = b.w;
        boxes[4 * i + 2] = b.x; boxes[4 * i + 3] = b.y;
        status[i] = im->h_status[(size_t)i];
    }
    return CEL_OK;
}

int cel_photon_split(cel_images *im, cel_sources *src, uint64_t seed, const int64_t *offsets, double *samp,
                     int mem, double *noise) {
    if (!im || !src) return fail(CEL_ERR_INVALID, "cel_photon_split: null argument");
    const bool resident = (offsets == nullptr);
    if (!resident && !samp) return fail(CEL_ERR_INVALID, "cel_photon_split: offsets given without an output buffer");
    if (!im->have_nelec) return fail(CEL_ERR_INVALID, "cel_photon_split needs cel_images_set_nelec first");
    { int rm = refuse_masked_unless_honoured(im, "cel_photon_split"); if (rm) return rm; }
    if (im->TW * im->TH != 2048) return fail(CEL_ERR_INVALID, "cel_photon_split needs 2048-pixel render tiles");
    cel_ctx *c = im->ctx;
    if (src->ctx != im->ctx || src->B != im->B) return fail(CEL_ERR_INVALID, "sources do not match images");
    HIP_TRY(hipSetDevice(c->device));
    // records + tile lists for exactly these sources come from a render.  Recurrence form: that
    // render is the one the split needs anyway -- every pixel's total rate, an image of its own
    // with the split's strict boxes (the model image of cel_images_get_lambda is left alone).
    // Direct form: a plain render (its kernel accumulates the totals itself).
    const bool hw = (c->variant != 0) && (im->TW == HW_TW);
    im->split_begins(hw);
    // a masked set under CEL_OPT_HONOUR_MASK: the masked twins (no photons, no sky, no draws at a masked pixel), no mass short cut
    const bool masked = honours_mask(im);
    bool use_massfx = false;
    const double *full_rate = nullptr;
    int rc;
    if (hw) {
        const int64_t npix = (int64_t)im->B * im->H * im->W;
        HIP_TRY(im->d_rate.grow(npix, npix, c->stream));
        const bool current = im->model_current(*src, c->render_T);
        if (c->split_full) {
            // CEL_OPT_SPLIT_FULL_BOX: a source takes part on its WHOLE box, so the totals are the model image itself -- the one
            // on the device when it is these sources', a render into the totals image otherwise
            if (c->split_reuse && current) { full_rate = im->d_lambda; rc = CEL_OK; }
            else rc = render_impl(im, src, 0, nullptr, nullptr, im->d_rate);
        } else if (c->split_reuse && current) {
            const int64_t nm = src->S * im->B;
            if (resident && c->mass_reuse_of() && nm > 0 && !masked) {
                // both kernels of this path also sum every unit stamp they evaluate: together the stamps' masses (cel_stamp_mass)
                if (nm > im->d_massfx.cap) {     // the two grow together; d_massfx, named last, holds the pair's capacity
                    const int64_t cap = nm + nm / 4 + 64;
                    HIP_TRY(grow_group(c->stream, im->d_mass_todo, cap + 1, im->d_massfx, cap));
                }
                HIP_TRY(hipMemsetAsync(im->d_massfx, 0, sizeof(unsigned long long) * nm, c->stream));
                use_massfx = true;
            }
            // the model image, records and tile lists of exactly these sources are on the device (the chain's trace render
            // came last): the totals are that image minus every source's first box row and column (k_border.h)
            RenderArgs a;
            memset(&a, 0, sizeof(a));
            a.bands = im->d_bands; a.recs = im->d_recs; a.lists = im->d_lists; a.tile_cnt = im->d_tile_cnt; a.tile_off = im->d_tile_off;
            a.lambda = im->d_lambda; a.S = src->S; a.capacity = im->d_lists.cap; a.B = im->B; a.H = im->H; a.W = im->W;
            a.ntx = im->ntx; a.nty = im->nty;
            int pi = prof_slot(c, CEL_K_TOTALS);
            LAUNCH_EV(k_strict_totals, dim3((unsigned)(im->B * im->ntx * im->nty)), dim3(64), c->stream, EV0(c, pi), EV1(c, pi), a, im->d_rate,
                      use_massfx ? im->d_massfx : (unsigned long long *)nullptr);
            HIP_TRY(hipGetLastError());
            rc = CEL_OK;
        } else {
            rc = render_impl(im, src, CEL_RENDER_STRICT, nullptr, nullptr, im->d_rate);
        }
    } else {
        rc = cel_render_field(im, src, 0, nullptr, nullptr);
    }
    if (rc) return rc;
    const int B = im->B;
    const int64_t S = src->S, n = S * B;
    const int T = B * im->ntx * im->nty;
    int64_t total = 0;
    int64_t *d_off = nullptr;
    void *d_samp = nullptr;             // resident: int32 photon counts; a caller's buffer: doubles
    if (resident) {
        // patch boxes + offsets laid out on the device; only the total size comes back
        if (n + 1 > im->d_sbox.cap) {
            const int64_t cap = n + n / 4 + 64, nb = cap / 1024 + 2;
            HIP_TRY(grow_group(c->stream, im->d_snz, cap, im->d_soff, cap, im->d_ssum, cap, im->d_nnz, cap, im->d_nzmode, cap,
                               im->d_nzoff, cap, im->d_btot, nb, im->d_sbox, cap));
        }
        {
            const unsigned nblk = (unsigned)((n + 1023) / 1024);
            hipLaunchKernelGGL(k_samp_layout, dim3(nblk), dim3(1024), 0, c->stream, im->d_recs, S, B, im->d_sbox, im->d_soff, im->d_btot);
            hipLaunchKernelGGL(k_scan_totals, dim3(1), dim3(1024), 0, c->stream, im->d_btot, (int)nblk, im->d_soff + n);
            hipLaunchKernelGGL(k_scan_apply, dim3(nblk), dim3(1024), 0, c->stream, im->d_soff, n, (const long long *)im->d_btot);
        }
        HIP_TRY(hipMemcpyAsync(&c->mail->sh.scan_total, im->d_soff + n, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        total = c->mail->sh.scan_total;
        HIP_TRY(im->d_samp.grow(total, total + total / 8 + 1024, c->stream));
        d_off = im->d_soff;
        d_samp = im->d_samp;
    } else {
        // the caller's layout against the sources' own boxes (cel_source_boxes): a patch too small for its box would be
        // written past its end
        if (offsets[0] != 0) return fail(CEL_ERR_INVALID, "cel_photon_split: offsets[0] must be 0");
        if ((rc = host_boxes(im, src))) return rc;
        for (int64_t sidx = 0; sidx < S; sidx++)
            for (int b = 0; b < B; b++) {
                const int4 bx = im->h_boxes[(size_t)((int64_t)b * S + sidx)];
                const int64_t area = (im->h_status[(size_t)((int64_t)b * S + sidx)] > 0) ? (int64_t)(bx.y - bx.x) * (bx.w - bx.z) : 0;
                const int64_t i = sidx * B + b;
                if (offsets[i + 1] - offsets[i] != area)
                    return fail(CEL_ERR_INVALID, "cel_photon_split: offsets give source %lld band %d %lld values, its box has %lld pixels (cel_source_boxes)",
                                (long long)sidx, b, (long long)(offsets[i + 1] - offsets[i]), (long long)area);
            }
        total = offsets[n];
        if ((rc = scratch_get(c, SCR_OFFSETS, sizeof(int64_t) * (n + 1), (void **)&d_off))) return rc;
        HIP_TRY(hipMemcpyAsync(d_off, offsets, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, c->stream));
        if (mem == CEL_DEVICE) d_samp = samp;
        else if ((rc = scratch_get(c, SCR_PATCH_DATA, sizeof(double) * (total > 0 ? total : 1), &d_samp))) return rc;
    }
    // resident + recurrence form: the kernel writes every interior pixel and reduces the photon
    // rectangles itself; otherwise zero the buffer and (resident) find the rectangles afterwards
    const bool fused_nz = resident && hw && n > 0;
    if (resident) im->split_laid_out(S, total, fused_nz);
    // photon lists: pixel coordinates are packed into 16 bits each
    const bool lists = fused_nz && im->W < 65536 && (im->win_y0 + im->H) < 65536 && c->nz_force != 2;
    if (fused_nz) HIP_TRY(hipMemsetAsync(im->d_ssum, 0, sizeof(double) * n, c->stream));
    if (lists) HIP_TRY(hipMemsetAsync(im->d_nnz, 0, sizeof(int) * n, c->stream));
    if (fused_nz)
        hipLaunchKernelGGL(k_samp_prepare<int>, dim3((unsigned)((n + 4 * SAMP_PREP_PER_WAVE - 1) / (4 * SAMP_PREP_PER_WAVE))), dim3(256), 0, c->stream,
                           im->d_sbox, im->d_soff, im->d_samp, im->d_snz, n);
    else if (total > 0)
        HIP_TRY(hipMemsetAsync(d_samp, 0, (resident ? sizeof(int) : sizeof(double)) * total, c->stream));
    {
        SplitArgs a;
        a.bands = im->d_bands; a.recs = im->d_recs; a.lists = im->d_lists; a.tile_cnt = im->d_tile_cnt;
        a.tile_off = im->d_tile_off; a.nelec = im->d_nelec; a.offsets = d_off; a.samp = d_samp;
        a.partials = im->d_partials; a.S = S; a.capacity = im->d_lists.cap; a.B = B; a.H = im->H; a.W = im->W;
        a.ntx = im->ntx; a.nty = im->nty; a.TW = im->TW; a.TH = im->TH; a.seed = seed;
        a.win_y0 = im->win_y0; a.full_H = im->full_H;
        a.noise_y0 = im->noise_y0; a.noise_y1 = im->noise_y1;
        a.rate_img = full_rate ? full_rate : im->d_rate; a.tail_T = c->tail_T; a.nz = fused_nz ? im->d_snz : nullptr;
        a.strict = c->split_full ? 0 : 1;
        im->split_totals_from_model(full_rate != nullptr);
        a.order = (hw && tile_order_of(c, im)) ? im->d_order : nullptr;
        a.sums = fused_nz ? im->d_ssum : nullptr;
        a.nnz = lists ? im->d_nnz : nullptr;
        a.massfx = (use_massfx && hw && resident) ? im->d_massfx : nullptr;
        a.debug = c->debug;
        if (hw && (rc = scratch_get(c, SCR_VALUES, sizeof(double) * 2 * (size_t)T, (void **)&a.partials))) return rc;
        int pi = prof_begin(c, CEL_K_SPLIT);
        if (masked) {          // (a set with a NaN never takes the 16-bit photons-left plane: nelec_u16 is false)
            if (hw && resident) hipLaunchKernelGGL(k_photon_split_hw_masked<int>, dim3(2 * T), dim3(64), 0, c->stream, a);
            else if (hw) hipLaunchKernelGGL(k_photon_split_hw_masked<double>, dim3(2 * T), dim3(64), 0, c->stream, a);
            else if (resident) hipLaunchKernelGGL(k_photon_split_masked<int>, dim3(T), dim3(64), 0, c->stream, a);
            else hipLaunchKernelGGL(k_photon_split_masked<double>, dim3(T), dim3(64), 0, c->stream, a);
        } else if (hw && resident) {
            if (im->nelec_u16) hipLaunchKernelGGL((k_photon_split_hw<int, unsigned short>), dim3(2 * T), dim3(64), 0, c->stream, a);
            else hipLaunchKernelGGL((k_photon_split_hw<int, int>), dim3(2 * T), dim3(64), 0, c->stream, a);
        } else if (hw) {
            if (im->nelec_u16) hipLaunchKernelGGL((k_photon_split_hw<double, unsigned short>), dim3(2 * T), dim3(64), 0, c->stream, a);
            else hipLaunchKernelGGL((k_photon_split_hw<double, int>), dim3(2 * T), dim3(64), 0, c->stream, a);
        }
        else if (resident) hipLaunchKernelGGL(k_photon_split<int>, dim3(T), dim3(64), 0, c->stream, a);
        else hipLaunchKernelGGL(k_photon_split<double>, dim3(T), dim3(64), 0, c->stream, a);
        prof_end(c, pi);
        hipLaunchKernelGGL(k_reduce, dim3(B), dim3(256), 0, c->stream, a.partials, (hw ? 2 : 1) * im->ntx * im->nty, im->d_llband,
                           (hw ? 2 : 1) * im->ntx * im->nty, 0, 1);
        if (resident && n > 0 && !fused_nz)   // where each patch's photons are: the conditional likelihoods evaluate only there
            hipLaunchKernelGGL(k_patch_nzbox<int>, dim3((unsigned)n), dim3(64), 0, c->stream, im->d_sbox, im->d_soff, (const int *)im->d_samp, im->d_snz);
    }
    if (lists)      // where each patch's photon list starts, and whether its likelihood is cheaper at the photons or densely
    {
        const unsigned nblk = (unsigned)((n + 1023) / 1024);
        hipLaunchKernelGGL(k_nz_layout, dim3(nblk), dim3(1024), 0, c->stream, (const int *)im->d_nnz, (const int4 *)im->d_snz,
                           (const int *)src->d_type, S, B, c->nz_force, c->nz_bias, im->d_nzoff, im->d_nzmode, im->d_btot);
        hipLaunchKernelGGL(k_scan_totals, dim3(1), dim3(1024), 0, c->stream, im->d_btot, (int)nblk, im->d_nzoff + n);
        hipLaunchKernelGGL(k_scan_apply, dim3(nblk), dim3(1024), 0, c->stream, im->d_nzoff, n, (const long long *)im->d_btot);
    }
    HIP_TRY(hipMemcpyAsync(c->mail->ll_band, im->d_llband, sizeof(double) * B, hipMemcpyDeviceToHost, c->stream));
    if (lists) HIP_TRY(hipMemcpyAsync(&c->mail->sh.scan_total, im->d_nzoff + n, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (fused_nz) {
        // what a Gibbs sweep asks for next (the photons per source: the flux and sky steps; the patch areas) rides back now:
        // cel_samples_fetch then needs no wait of its own, and the list compaction queued below runs under the host's work
        if (n + 1 > im->h_ssum.cap) {
            const int64_t cap = n + n / 4 + 64;
            HIP_TRY(grow_group(c->stream, im->h_soff, cap, im->h_ssum, cap));
        }
        HIP_TRY(hipMemcpyAsync(im->h_ssum, im->d_ssum, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(im->h_soff, im->d_soff, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost, c->stream));
    }
    if (!resident && mem != CEL_DEVICE && total > 0)
        HIP_TRY(hipMemcpyAsync(samp, d_samp, sizeof(double) * total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    im->split_ends(fused_nz, (use_massfx && hw && resident) ? src->gen : 0, c->tail_T);
    if (noise) for (int b = 0; b < B; b++) noise[b] = c->mail->ll_band[b];
    if (lists) {
        const int64_t nn = c->mail->sh.scan_total;
        HIP_TRY(im->d_nzlist.grow(nn, nn + nn / 4 + 1024, c->stream));
        // stream-ordered: whatever scores against these patches next runs behind it
        hipLaunchKernelGGL(k_nz_compact, dim3((unsigned)n), dim3(64), 0, c->stream, (const int4 *)im->d_sbox, (const int64_t *)im->d_soff,
                           (const int *)im->d_samp, (const int4 *)im->d_snz, (const int64_t *)im->d_nzoff, im->d_nzlist);
        HIP_TRY(hipGetLastError());
        im->split_lists_built();
    }
    return CEL_OK;
}

int cel_samples_info(cel_images *im, int64_t *S, int64_t *total) {
    if (!im || !S || !total) return fail(CEL_ERR_INVALID, "cel_samples_info: null argument");
    *S = im->split.samp_S;
    *total = im->split.samp_total;
    return CEL_OK;
}

int cel_samples_fetch(cel_images *im, int32_t *boxes, int64_t *offsets, double *data, double *sums) {
    if (!im) return fail(CEL_ERR_INVALID, "cel_samples_fetch: null argument");
    if (im->split.samp_S <= 0) return fail(CEL_ERR_INVALID, "no resident photon split: call cel_photon_split with offsets = NULL first");
    cel_ctx *c = im->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int64_t n = im->split.samp_S * im->B;
    int rc = CEL_OK;
    if (!boxes && !data && im->split.hsum_valid && n + 1 <= im->h_ssum.cap) {        // host copies made by the split itself: no wait
        if (offsets) memcpy(offsets, im->h_soff, sizeof(int64_t) * (n + 1));
        if (sums) memcpy(sums, im->h_ssum, sizeof(double) * n);
        return CEL_OK;
    }
    if (boxes) {
        std::vector<int4> hb((size_t)n);
        if ((rc = copy_out(hb.data(), im->d_sbox, sizeof(int4) * n, CEL_HOST, c->stream))) return rc;
        for (int64_t i = 0; i < n; i++) {
            boxes[4 * i] = hb[i].z; boxes[4 * i + 1] = hb[i].w; boxes[4 * i + 2] = hb[i].x; boxes[4 * i + 3] = hb[i].y;
        }
    }
    if (offsets && (rc = copy_out(offsets, im->d_soff, sizeof(int64_t) * (n + 1), CEL_HOST, c->stream))) return rc;
    if (data && im->split.samp_total > 0) {           // int32 on the device, doubles across the ABI
        std::vector<int> hs((size_t)im->split.samp_total);
        if ((rc = copy_out(hs.data(), im->d_samp, sizeof(int) * im->split.samp_total, CEL_HOST, c->stream))) return rc;
        for (int64_t i = 0; i < im->split.samp_total; i++) data[i] = (double)hs[(size_t)i];
    }
    if (sums) {
        if (im->split.ssum_valid) {       // the split kernel summed them itself (exact: integer-valued)
            if ((rc = copy_out(sums, im->d_ssum, sizeof(double) * n, CEL_HOST, c->stream))) return rc;
        } else {
            double *d_sums = nullptr;
            if ((rc = scratch_get(c, SCR_PATCH_DATA, sizeof(double) * n, (void **)&d_sums))) return rc;
            hipLaunchKernelGGL(k_patch_sums<int>, dim3((unsigned)n), dim3(256), 0, c->stream, im->d_soff, (const int *)im->d_samp, d_sums);
            if ((rc = copy_out(sums, d_sums, sizeof(double) * n, CEL_HOST, c->stream))) return rc;
        }
    }
    return CEL_OK;
}

int cel_samples_photon_rects(cel_images *im, int32_t *rects) {
    if (!im || !rects) return fail(CEL_ERR_INVALID, "cel_samples_photon_rects: null argument");
    if (im->split.samp_S <= 0 || !im->d_snz)
        return fail(CEL_ERR_INVALID, "no resident photon split: call cel_photon_split with offsets = NULL first");
    cel_ctx *c = im->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int64_t n = im->split.samp_S * im->B;
    std::vector<int4> hb((size_t)n);
    int rc = copy_out(hb.data(), im->d_snz, sizeof(int4) * n, CEL_HOST, c->stream);
    if (rc) return rc;
    for (int64_t i = 0; i < n; i++) {
        const bool held = hb[i].y > hb[i].x && hb[i].w > hb[i].z;         // (the kernels mark an empty patch in two ways)
        rects[4 * i] = held ? hb[i].z : 0; rects[4 * i + 1] = held ? hb[i].w : 0;
        rects[4 * i + 2] = held ? hb[i].x : 0; rects[4 * i + 3] = held ? hb[i].y : 0;
    }
    return CEL_OK;
}

// cel_slice_sample(param = CEL_SLICE_MOMENTS).  Reads the split (patches or photon lists, behind whatever the split left queued on
// the stream) and writes the caller's array: no stamp of the set changes.  src may be null (the split's own S).
static int samples_moments(cel_images *im, const cel_sources *src, int64_t *mom) {
    if (!mom) return fail(CEL_ERR_INVALID, "cel_slice_sample: the moments (param 10) need stats[S * B * 6]");
    if (src) {
        if (src->B != im->B || src->ctx != im->ctx) return fail(CEL_ERR_INVALID, "sources do not match images");
        int rs = need_resident_split(im, src, "cel_slice_sample"); if (rs) return rs;
    } else if (im->split.samp_S <= 0) {     // (need_resident_split's words; no catalogue was named, so no count of `these`)
        return fail(CEL_ERR_INVALID, "cel_slice_sample needs a resident photon split (have %lld sources' patches)", (long long)im->split.samp_S);
    }
    cel_ctx *c = im->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int64_t n = im->split.samp_S * im->B;
    if (n * MOM_PARTS > 0x7fffffffLL) return fail(CEL_ERR_INVALID, "cel_slice_sample: too many (source, band) jobs for one launch of the moments");
    long long *d_mom = nullptr;
    int rc = scratch_get(c, SCR_PATCH_DATA, sizeof(long long) * 6 * n, (void **)&d_mom);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d_mom, 0, sizeof(long long) * 6 * n, c->stream));
    const bool use_nz = im->split.nz_valid && c->variant != 0;      // the likelihoods' rule (patch_ll_resident, the samplers)
    hipLaunchKernelGGL(k_moments, dim3((unsigned)(n * MOM_PARTS)), dim3(64), 0, c->stream, n, (const int4 *)im->d_sbox,
                       (const int64_t *)im->d_soff, (const int *)im->d_samp, use_nz ? (const int *)im->d_nzmode : (const int *)nullptr,
                       (const int64_t *)im->d_nzoff, (const NzEntry *)im->d_nzlist, d_mom);
    HIP_TRY(hipGetLastError());
    static_assert(sizeof(long long) == sizeof(int64_t), "the kernel's sums are the ABI's int64");
    return copy_out(mom, d_mom, sizeof(int64_t) * 6 * n, CEL_HOST, c->stream);
}

int cel_debug_binomial(cel_ctx *c, int64_t n, double p, uint64_t seed, int64_t N, int64_t *out) {
    if (!c || !out || N < 0 || n < 0) return fail(CEL_ERR_INVALID, "cel_debug_binomial: bad argument");
    if (N == 0) return CEL_OK;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<long long> d;
    HIP_TRY(d.grow(N, N, c->stream));
    hipLaunchKernelGGL(k_binomial_draws, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, (long long)n, p,
                       (unsigned long long)seed, N, d);
    return copy_out(out, d, sizeof(long long) * N, CEL_HOST, c->stream);
}

// ---- E-step statistics -------------------------------------------------------------------------
int cel_estep_stats(cel_images *im, cel_sources *src, double *xtilde, double *mass, double *noise) {
    if (!im || !src) return fail(CEL_ERR_INVALID, "cel_estep_stats: null argument");
    if (!im->have_nelec) return fail(CEL_ERR_INVALID, "cel_estep_stats needs cel_images_set_nelec first");
    cel_ctx *c = im->ctx;
    // lambda for exactly these sources must be resident (this also runs k_prep for them)
    int rc = render_impl(im, src, CEL_RENDER_KEEP_LISTS, nullptr, nullptr, nullptr);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int B = im->B;
    const int64_t S = src->S;
    const int nblk = im->ntx * im->nty;                 // d_partials holds B * nblk doubles
    im->partials_overwritten();                         // ... of this call's sky term from here on
    double *d_x = nullptr, *d_m = nullptr, *d_part = nullptr;
    // recurrence evaluator on the 32 x 64 layout: the tile-walking form (the render above left the
    // lists and boxes of exactly these sources on the device); CEL_OPT_DEBUG bit 64 keeps the per-source form
    const bool tiles = (c->variant != 0) && (im->TW == HW_TW) && !(c->debug & 64) && S > 0;
    std::vector<double> hx((size_t)(S * B)), hm((size_t)(S * B));
    if (S > 0) {
        // the context's scratch arena, not an allocation per call: EM iterates this
        if ((rc = scratch_get(c, SCR_TMP_A, sizeof(double) * S * B, (void **)&d_x)) ||
            (rc = scratch_get(c, SCR_TMP_B, sizeof(double) * S * B, (void **)&d_m))) return rc;
        if (tiles && (rc = scratch_get(c, SCR_TMP_C, sizeof(double) * 2 * (size_t)im->d_lists.cap, (void **)&d_part))) return rc;
        int pi = prof_begin(c, CEL_K_ESTEP);
        const bool masked = im->any_masked;     // the masked twins (k_estep.h): an unmasked set takes the kernels it always took
        if (c->variant == 0)
            hipLaunchKernelGGL((masked ? k_estep_src_masked : k_estep_src), dim3((unsigned)(S * B)), dim3(256), 0, c->stream, im->d_bands, B, im->H, im->W,
                               S, im->d_recs, im->d_nelec, im->d_lambda, d_x, d_m);
        else if (tiles) {
            // walk the render tiles: nelec / lambda are read once, every list entry gets its pair of sums,
            // the gather adds a source's entries in tile order
            EstepArgs ea;
            ea.bands = im->d_bands; ea.recs = im->d_recs; ea.lists = im->d_lists; ea.tile_cnt = im->d_tile_cnt;
            ea.tile_off = im->d_tile_off; ea.order = tile_order_of(c, im) ? im->d_order : nullptr;
            ea.nelec = im->d_nelec; ea.lambda = im->d_lambda; ea.partial = d_part; ea.noise_partial = im->d_partials;
            ea.S = S; ea.capacity = im->d_lists.cap; ea.B = B; ea.H = im->H; ea.W = im->W; ea.ntx = im->ntx; ea.nty = im->nty;
            ea.tail_T = c->tail_T;
            hipLaunchKernelGGL((masked ? k_estep_tiles_masked : k_estep_tiles), dim3((unsigned)(B * nblk)), dim3(64), 0, c->stream, ea);
            hipLaunchKernelGGL(k_estep_gather, dim3((unsigned)((S * B + 255) / 256)), dim3(256), 0, c->stream, im->d_boxes, im->d_kind,
                               S, B, im->ntx, im->nty, im->d_tile_cnt, im->d_tile_nstar, im->d_tile_off, im->d_lists, im->d_lists.cap,
                               d_part, d_x, d_m);
        } else
            hipLaunchKernelGGL((masked ? k_estep_src_hw_masked : k_estep_src_hw), dim3((unsigned)(S * B)), dim3(64), 0, c->stream, im->d_bands, B, im->H, im->W,
                               S, im->d_recs, im->d_nelec, im->d_lambda, c->tail_T, d_x, d_m);
        prof_end(c, pi);
        HIP_TRY(hipMemcpyAsync(hx.data(), d_x, sizeof(double) * S * B, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(hm.data(), d_m, sizeof(double) * S * B, hipMemcpyDeviceToHost, c->stream));
    }
    if (!tiles)      // the tile walk has left the sky term's per-tile sums in d_partials
        hipLaunchKernelGGL((im->any_masked ? k_estep_noise_masked : k_estep_noise), dim3(B * nblk), dim3(256), 0, c->stream, im->d_bands, (int64_t)im->H * im->W, nblk,
                           im->d_nelec, im->d_lambda, im->d_partials);
    hipLaunchKernelGGL(k_reduce, dim3(B), dim3(256), 0, c->stream, im->d_partials, nblk, im->d_llband, nblk, 0, 1);
    HIP_TRY(hipMemcpyAsync(c->mail->ll_band, im->d_llband, sizeof(double) * B, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (xtilde) memcpy(xtilde, hx.data(), sizeof(double) * S * B);
    if (mass) memcpy(mass, hm.data(), sizeof(double) * S * B);
    if (noise) for (int b = 0; b < B; b++) noise[b] = c->mail->ll_band[b];
    return CEL_OK;
}

// ---- gradient of the field log-likelihood (k_grad.h) --------------------------------------------
int cel_loglik_grad(cel_images *im, cel_sources *src, double *ll_total, double *g_radec, double *g_counts, double *g_shape,
                    int mem) {
    if (!im || !src) return fail(CEL_ERR_INVALID, "cel_loglik_grad: null argument");
    if (!im->have_nelec) return fail(CEL_ERR_INVALID, "cel_loglik_grad needs cel_images_set_nelec first");
    if (im->win_y0 != 0 || im->full_H != im->H)
        return fail(CEL_ERR_INVALID, "cel_loglik_grad: an image set with a row window (cel_images_set_window) is not supported");
    if (mem != CEL_HOST && mem != CEL_DEVICE) return fail(CEL_ERR_INVALID, "cel_loglik_grad: bad mem");
    cel_ctx *c = im->ctx;
    // lambda, records and boxes of exactly these sources; the log-likelihood is cel_render_field's own
    double ll = 0.0;
    int rc = render_impl(im, src, CEL_RENDER_LOGLIK, nullptr, &ll, nullptr);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int B = im->B;
    const int64_t S = src->S;
    if (S > 0 && (g_radec || g_counts || g_shape)) {
        double *d_sums = nullptr, *d_out = nullptr;
        if ((rc = scratch_get(c, SCR_TMP_A, sizeof(double) * GRAD_NS * S * B, (void **)&d_sums))) return rc;
        double *o_radec = g_radec, *o_counts = g_counts, *o_shape = g_shape;
        if (mem != CEL_DEVICE) {
            if ((rc = scratch_get(c, SCR_TMP_B, sizeof(double) * (size_t)S * (6 + B), (void **)&d_out))) return rc;
            o_radec = g_radec ? d_out : nullptr;
            o_shape = g_shape ? d_out + 2 * S : nullptr;
            o_counts = g_counts ? d_out + 6 * S : nullptr;
        }
        int pi = prof_begin(c, CEL_K_GRAD);
        hipLaunchKernelGGL((im->any_masked ? k_grad_src_masked : k_grad_src), dim3((unsigned)(S * B)), dim3(64), 0, c->stream, im->d_bands, B, im->H, im->W, S,
                           im->d_recs, im->d_nelec, im->d_lambda, c->tail_T, d_sums);
        hipLaunchKernelGGL(k_grad_chain, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, c->stream, im->d_bands, B, S,
                           im->d_recs, src->d_type, src->d_shape, src->d_counts, d_sums, o_radec, o_counts, o_shape);
        prof_end(c, pi);
        HIP_TRY(hipGetLastError());
        if (mem != CEL_DEVICE) {
            if (g_radec) HIP_TRY(hipMemcpyAsync(g_radec, o_radec, sizeof(double) * 2 * S, hipMemcpyDeviceToHost, c->stream));
            if (g_shape) HIP_TRY(hipMemcpyAsync(g_shape, o_shape, sizeof(double) * 4 * S, hipMemcpyDeviceToHost, c->stream));
            if (g_counts) HIP_TRY(hipMemcpyAsync(g_counts, o_counts, sizeof(double) * S * B, hipMemcpyDeviceToHost, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (ll_total) *ll_total = ll;
    return CEL_OK;
}

// ---- generic evaluator ------------------------------------------------------------------------
int cel_gmm_like_2d(cel_ctx *c, const double *x, int64_t N, const double *ws, const double *mus,
                    const double *sigs, int K, double *probs, int mem) {
    if (!c || !x || !ws || !mus || !sigs || !probs) return fail(CEL_ERR_INVALID, "cel_gmm_like_2d: null argument");
    if (N < 0 || K < 1) return fail(CEL_ERR_INVALID, "Means, covariances and weights must have same first dimension!");
    if (N == 0) return CEL_OK;
    HIP_TRY(hipSetDevice(c->device));
    // gmm_like_fast.pyx:162-176: det, inverse and the normaliser are per-component scalars
    std::vector<double> comp((size_t)K * 6);
    const double log2pi = log(2.0 * PI_D);
    for (int k = 0; k < K; k++) {
        const double *s = sigs + 4 * k;
        double det = s[0] * s[3] - s[1] * s[2];
        comp[6 * k + 0] = exp(-log2pi - 0.5 * log(det)) * ws[k];
        comp[6 * k + 1] = mus[2 * k];
        comp[6 * k + 2] = mus[2 * k + 1];
        comp[6 * k + 3] = s[3] / det;
        comp[6 * k + 4] = -1 * s[1] / det;
        comp[6 * k + 5] = s[0] / det;
    }
    DevBuf<double> d_comp, bx, bp;      // per call; a caller's host arrays are staged in bx / bp
    HIP_TRY(d_comp.grow(6 * K, 6 * K, c->stream));
    HIP_TRY(hipMemcpyAsync(d_comp, comp.data(), sizeof(double) * 6 * K, hipMemcpyHostToDevice, c->stream));
    double *d_x = const_cast<double *>(x), *d_p = probs;
    if (mem != CEL_DEVICE) {
        HIP_TRY(bx.grow(2 * N, 2 * N, c->stream));
        HIP_TRY(bp.grow(N, N, c->stream));
        HIP_TRY(hipMemcpyAsync(bx, x, sizeof(double) * 2 * N, hipMemcpyHostToDevice, c->stream));
        d_x = bx; d_p = bp;
    }
    {
        int pi = prof_begin(c, CEL_K_GMM);
        hipLaunchKernelGGL(k_gmm, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, d_x, N, d_comp, K, d_p);
        prof_end(c, pi);
    }
    HIP_TRY(hipGetLastError());
    if (mem != CEL_DEVICE) HIP_TRY(hipMemcpyAsync(probs, d_p, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CEL_OK;
}

int cel_mog_loglike(cel_ctx *c, const double *x, int64_t N, const double *means, const double *icovs,
                    const double *logw, int K, double *out, int mem) {
    if (!c || !x || !means || !icovs || !logw || !out) return fail(CEL_ERR_INVALID, "cel_mog_loglike: null argument");
    if (N < 0 || K < 1) return fail(CEL_ERR_INVALID, "cel_mog_loglike: bad sizes");
    if (N == 0) return CEL_OK;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<double> comp((size_t)K * 6);
    for (int k = 0; k < K; k++) {
        comp[6 * k + 0] = logw[k];
        comp[6 * k + 1] = means[2 * k];
        comp[6 * k + 2] = means[2 * k + 1];
        comp[6 * k + 3] = icovs[4 * k];
        comp[6 * k + 4] = icovs[4 * k + 1] + icovs[4 * k + 2];     // the einsum keeps both off-diagonal terms (mog.py:15-16)
        comp[6 * k + 5] = icovs[4 * k + 3];
    }
    double *d_comp = nullptr, *d_x = nullptr, *d_o = nullptr;
    int rc;
    if ((rc = scratch_get(c, SCR_TMP_A, sizeof(double) * 6 * K, (void **)&d_comp))) return rc;
    HIP_TRY(hipMemcpyAsync(d_comp, comp.data(), sizeof(double) * 6 * K, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));      // comp is a local
    if (mem == CEL_DEVICE) {
        d_x = const_cast<double *>(x);
        d_o = out;
    } else {
        if ((rc = scratch_get(c, SCR_TMP_B, sizeof(double) * 2 * N, (void **)&d_x)) ||
            (rc = scratch_get(c, SCR_TMP_C, sizeof(double) * N, (void **)&d_o))) return rc;
        HIP_TRY(hipMemcpyAsync(d_x, x, sizeof(double) * 2 * N, hipMemcpyHostToDevice, c->stream));
    }
    int pi = prof_begin(c, CEL_K_GMM);
    hipLaunchKernelGGL(k_mog_ll, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, d_x, N, d_comp, K, d_o);
    prof_end(c, pi);
    HIP_TRY(hipGetLastError());
    if (mem != CEL_DEVICE) HIP_TRY(hipMemcpyAsync(out, d_o, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CEL_OK;
}

int cel_galaxy_mixture_params(cel_ctx *c, int64_t N, const double *W, const double *v_s, const double *image_ws,
                              const double *image_means, const double *image_covars, int K_psf, const double *amp,
                              const double *sigs, int J, double *weights, double *means, double *covars) {
    if (!c || !W || !v_s || !image_ws || !image_means || !image_covars || !amp || !sigs || !weights || !means || !covars)
        return fail(CEL_ERR_INVALID, "cel_galaxy_mixture_params: null argument");
    if (N < 0 || K_psf < 1 || J < 1 || K_psf > 4096 || J > 4096) return fail(CEL_ERR_INVALID, "cel_galaxy_mixture_params: bad sizes");
    if (N == 0) return CEL_OK;
    HIP_TRY(hipSetDevice(c->device));
    const int64_t K = (int64_t)K_psf * J, n = N * K;
    // inputs in one upload: W (4N), v_s (2N), ws (Kp), means (2Kp), covars (4Kp), amp (J), sigs (J)
    const size_t nin = (size_t)(6 * N + 7 * K_psf + 2 * J);
    std::vector<double> hin(nin);
    double *q = hin.data();
    memcpy(q, W, sizeof(double) * 4 * N); q += 4 * N;
    memcpy(q, v_s, sizeof(double) * 2 * N); q += 2 * N;
    memcpy(q, image_ws, sizeof(double) * K_psf); q += K_psf;
    memcpy(q, image_means, sizeof(double) * 2 * K_psf); q += 2 * K_psf;
    memcpy(q, image_covars, sizeof(double) * 4 * K_psf); q += 4 * K_psf;
    memcpy(q, amp, sizeof(double) * J); q += J;
    memcpy(q, sigs, sizeof(double) * J);
    double *d_in = nullptr, *d_out = nullptr;
    int rc;
    if ((rc = scratch_get(c, SCR_TMP_A, sizeof(double) * nin, (void **)&d_in)) ||
        (rc = scratch_get(c, SCR_TMP_B, sizeof(double) * 7 * n, (void **)&d_out))) return rc;
    HIP_TRY(hipMemcpyAsync(d_in, hin.data(), sizeof(double) * nin, hipMemcpyHostToDevice, c->stream));
    const double *dW = d_in, *dv = dW + 4 * N, *dws = dv + 2 * N, *dmu = dws + K_psf, *dcv = dmu + 2 * K_psf,
                 *damp = dcv + 4 * K_psf, *dsig = damp + J;
    hipLaunchKernelGGL(k_mixture_params, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, N, dW, dv, dws, dmu, dcv,
                       K_psf, damp, dsig, J, d_out, d_out + n, d_out + 3 * n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(weights, d_out, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(means, d_out + n, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(covars, d_out + 3 * n, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return CEL_OK;
}

int cel_bounding_radius(const double *w, const double *mu, const double *cov, int K, double error,
                        const double *center, double *out) {
    (void)w;
    if (!mu || !cov || !out || K < 1) return fail(CEL_ERR_INVALID, "cel_bounding_radius: bad argument");
    if (!(error > 0.0 && error < 1.0)) return fail(CEL_ERR_INVALID, "error must be in (0,1)");
    *out = host_bounding_radius(mu, cov, K, error, center);
    return CEL_OK;
}

// ---- measurement ------------------------------------------------------------------------------
int cel_profile_reset(cel_ctx *c) {
    if (!c) return fail(CEL_ERR_INVALID, "null context");
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->prof.head = 0;
    c->prof.count = 0;
    for (int k = 0; k < CEL_K_COUNT; k++) { c->prof.sum_ms[k] = 0.0; c->prof.n[k] = 0; c->prof.seen[k] = 0; }
    return CEL_OK;
}

int cel_profile_get(cel_ctx *c, int kernel, double *mean_ms, int64_t *launches) {
    if (!c || kernel < 0 || kernel >= CEL_K_COUNT) return fail(CEL_ERR_INVALID, "cel_profile_get: bad argument");
    HIP_TRY(hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (mean_ms) *mean_ms = c->prof.n[kernel] ? c->prof.sum_ms[kernel] / (double)c->prof.n[kernel] : 0.0;
    if (launches) *launches = c->prof.n[kernel];
    return CEL_OK;
}

}  // extern "C"
