// field_state.h -- the stamps that vouch for what the library keeps between calls, and the only code that writes them
// (host code only; no HIP type in it: a test compiles it with the host compiler alone).
//
// A catalogue (SourceStamps, the base of cel_sources) says which generation of which object it is.  An image set (FieldState,
// the base of cel_images) says whose records, tile lists, model image and photon split lie in its buffers.  Every short cut --
// the dirty-tile render, the split's totals from the resident model image, the masses off the split's sums, the star-only
// kernels, cel_stamp_mass_end -- asks a predicate here; every entry point that changes a buffer fires an event here.  What an
// event makes stale is written once, in the event (DESIGN.md carries the same table).
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <vector>

inline std::atomic<uint64_t> g_source_gen{0};   // process-wide: generations and object ids; bumped here and nowhere else

struct SourceStamps {
    uint64_t gen = 0;              // changes with every change of the catalogue on the device
    uint64_t uid = 0;              // which catalogue object this is (never reused: a generation alone does not say whose it is)
    uint64_t full_gen = 0;         // ... the generation of the last change of the WHOLE catalogue (cel_sources_set, a sampler's update)
    std::vector<uint64_t> row_gen; // per row: the generation of its last change by cel_sources_set_rows (empty: none since full_gen)
    int64_t n_gal = -1;            // entries that are not stars (type != 0); -1 = unknown (types written on the device)
    std::vector<int32_t> h_type;   // the types as the host last knew them (rows_replaced keeps n_gal exact with them)

    void created() { uid = ++g_source_gen; }
    // every row may have changed (cel_sources_set, a device sampler, a proposal set): no row stamps.  types_unknown: the
    // device wrote the types as well, the host's copy is void
    void all_rows_changed(bool types_unknown) {
        gen = full_gen = ++g_source_gen;
        row_gen.clear();
        if (types_unknown) { n_gal = -1; h_type.clear(); }
    }
    // n rows of the catalogue's S replaced from the host: which rows changed since when.  A render whose image set still
    // holds the model image of an earlier generation of THIS catalogue renders only the tiles these rows' boxes touch
    void rows_replaced(int64_t S, int64_t n, const int32_t *idx, const int32_t *type) {
        if ((int64_t)h_type.size() == S) {
            for (int64_t i = 0; i < n; i++) {
                n_gal += (type[i] != 0) - (h_type[idx[i]] != 0);
                h_type[idx[i]] = type[i];
            }
        } else {
            n_gal = -1;
        }
        gen = ++g_source_gen;
        if ((int64_t)row_gen.size() != S) row_gen.assign((size_t)S, 0);
        for (int64_t i = 0; i < n; i++) row_gen[idx[i]] = gen;
    }
    // the host knows every type again (an upload from host memory, the type move's readback)
    void types_known(const int32_t *type, int64_t S) {
        h_type.assign(type, type + S);
        n_gal = 0;
        for (int64_t i = 0; i < S; i++) n_gal += (type[i] != 0);
    }
};

// k_prep's records, boxes and status words on the device, and the host copy of the boxes
struct RecordStamps {
    uint64_t recs_gen = 0, hbox_gen = 0;    // the catalogue generation they belong to (0: nobody's)
    int64_t last_S = 0;                     // sources of the last k_prep
    uint64_t comps_gen = 0;                 // the record generation the component cache (k_comps.h) was built from (0: of none)
    bool of(const SourceStamps &src) const { return src.gen != 0 && recs_gen == src.gen; }
    // the component cache holds the rows k_comps would build NOW from the records that stand in d_recs: it was built from records
    // of this generation, and nobody has written, re-allocated or disowned the records since (those events zero the stamp).  The
    // rows are a function of the records and the bands' PSF tables alone: no sky level, threshold, tile or kernel choice
    bool comps_of_records() const { return comps_gen != 0 && comps_gen == recs_gen; }
    bool host_boxes_of(const SourceStamps &src) const { return of(src) && hbox_gen == src.gen; }
};

// the tile lists, and the launch order sorted from the last render's measured tile durations
struct ListStamps {
    uint64_t lists_gen = 0;
    int64_t cost_S = -1;          // sources of the render whose tile durations d_tile_cost holds (-1: nothing measured yet)
    int64_t order_S = -1;         // d_order already holds the heaviest-first order of those costs (sorted behind that render's readback)
    // the lists, per-tile counts, offsets, star counts, work estimates, super-tile arrays and the saved cursor words were built
    // by a SUCCESSFUL binning of exactly the (box, kind) table that stands in d_boxes / d_kind now, for so many sources, in this
    // window, by the same binning form, and nobody has re-allocated or written any of them since (-1: not so).  With it a
    // render's binning kernels may return at once when k_prep found no box or kind to change (k_bin2.h); without it they bin
    int64_t binned_S = -1;
    bool binning_of(int64_t S) const { return S > 0 && binned_S == S; }
    bool costs_of(int64_t S) const { return cost_S == S; }
    bool order_ready(int64_t S) const { return order_S == S && cost_S == S; }
};

// the model image in d_lambda (full boxes, the current sky levels) and the per-tile Poisson partials formed against it
struct ModelStamps {
    uint64_t lambda_gen = 0;         // the catalogue generation it was rendered from (0: not valid)
    uint64_t lambda_uid = 0;         // the catalogue OBJECT whose generation that is (row stamps of the same object only)
    double lambda_T = -1.0;          // ... the drop threshold that image was rendered at
    int lambda_parts = 0;            // ... with so many blocks per tile
    uint64_t partials_gen = 0;       // d_partials holds the partials of this generation's render (0: not)
    int64_t last_dirty = -1;         // the last render was incremental (-2; -1: it rendered every tile)
};

// the resident photon split: its patches, sums and photon lists, and the stamp sums it left for cel_stamp_mass
struct SplitStamps {
    int64_t samp_S = 0, samp_total = 0;     // sources and photon-count values of the resident patches (0: no resident split)
    bool ssum_valid = false;                // d_ssum: the split kernel summed the patches itself
    bool hsum_valid = false;                // h_ssum / h_soff: host copies made inside cel_photon_split
    bool nz_valid = false;                  // the photon lists
    bool rate_in_lambda = false;            // the last split read its totals from the model image itself
    uint64_t split_epoch = 0;               // photon splits of this set so far
    uint64_t massfx_gen = 0;                // d_massfx holds the stamp sums of the catalogue of this generation (0: of none)
    double massfx_T = -1.0;                 // ... formed at this per-source drop threshold
    bool resident_of(int64_t S) const { return samp_S > 0 && samp_S == S; }
    // the stamp sums are this catalogue's, and they carry the drop rule the mass kernel would apply now
    bool sums_of(const SourceStamps &src, double tail_T) const { return src.gen != 0 && massfx_gen == src.gen && massfx_T == tail_T; }
    void drop() { samp_S = samp_total = 0; ssum_valid = hsum_valid = nz_valid = false; massfx_gen = 0; }
};

// the masses waiting between cel_stamp_mass_begin and _end
struct PendingMass {
    int64_t pending = -1;            // doubles waiting in `values` (-1: none)
    int64_t todo_S = -1;             // >= 0: _begin took the short cut on a catalogue of so many sources; _end finishes its leftovers
    uint64_t gen = 0, epoch = 0;     // the catalogue generation _begin summed, and the set's split_epoch then: what _end checks
    const int *todo_ptr = nullptr;   // the short cut's to-do list as _begin saw it (a split in between may have re-allocated it: not owned)
    double *values = nullptr;        // (points into a scratch slot of the context: not owned)
    void cancel() { pending = -1; todo_S = -1; }
    void begin(uint64_t g, uint64_t e, int64_t n, int64_t short_cut_S, const int *todo, double *v) {
        gen = g; epoch = e; pending = n; todo_S = short_cut_S; todo_ptr = todo; values = v;
    }
    // hands out what waits, once; false: nothing was begun
    bool take(int64_t *n, int64_t *short_cut_S) {
        if (pending < 0) return false;
        *n = pending; *short_cut_S = todo_S;
        cancel();
        return true;
    }
    // neither k_prep nor a photon split ran for anyone else since _begin
    bool intact(const RecordStamps &rec, const SplitStamps &split) const { return rec.recs_gen == gen && split.split_epoch == epoch; }
};

struct FieldState {
    RecordStamps rec;
    ListStamps lists;
    ModelStamps model;
    SplitStamps split;
    PendingMass mass;
    bool nelec_u16 = false;          // every observed pixel in 0 ... 65 535: the split's 16-bit photons-left plane
    bool nelec_shared = false;       // cel_images_device_ptrs handed the observed pixels' device pointer out

    // ---- what the short cuts ask ----
    // model image, tile lists and records are all of exactly this catalogue, the image rendered at the threshold a render
    // would take now: the split may take its totals from the image
    bool model_current(const SourceStamps &src, double render_T) const {
        return src.gen != 0 && model.lambda_gen == src.gen && model.lambda_T == render_T && lists.lists_gen == src.gen &&
               rec.recs_gen == src.gen;
    }
    // the image, lists, records (and, for a log-likelihood, partials) of an EARLIER generation of this catalogue object of S
    // sources, rendered at this threshold by one block per tile, with row stamps for everything since: the dirty-tile render
    // may start from them.  (The plan's own terms -- options, flags, kernel choice -- stay in plan_render.)
    bool incremental_base(const SourceStamps &src, int64_t S, double render_T, bool need_partials) const {
        return S == rec.last_S && model.lambda_gen != 0 && model.lambda_uid == src.uid && model.lambda_T == render_T &&
               model.lambda_parts == 1 && model.lambda_gen != src.gen && model.lambda_gen >= src.full_gen &&
               lists.lists_gen == model.lambda_gen && rec.recs_gen == model.lambda_gen && (int64_t)src.row_gen.size() == S &&
               (!need_partials || (model.partials_gen == model.lambda_gen && !nelec_shared));
    }

    // the records, boxes, kinds and status words in the tables are what a k_prep of exactly this catalogue generation of S
    // sources would store now, AND the tile lists with their counts, offsets and cursor words were binned from that table by
    // the last general render, which was of this generation: a general render may launch NO k_prep (the binning launch then
    // leaves everything as it is, k_prep_bin.h: BIN_LEAVE).  The records are a function of the catalogue's rows, the bands'
    // WCS and PSF tables, the window and S -- no sky level, pixel, threshold or kernel choice enters them -- so what falsifies
    // it is: any change of the catalogue (a new src.gen: cel_sources_set / _set_rows with whatever values, every sampler, the
    // flux step, the type move), another catalogue object or generation prepared or rendered into this set (records_written,
    // small_star_render: recs_gen is theirs), new_window, records_regrown, ANY k_prep outside a render (records_written drops
    // binned_S: it zeroed the cursor words; a partial or box-less one writes generation 0), a render that did not end well
    // (render_begins drops lists_gen, only render_succeeded sets it again; render_overflowed), lists_regrown,
    // bin_form_changed, and the option (CEL_OPT_INCREMENTAL = 0: never).  Another image set rendered from the same catalogue
    // changes no stamp here.  Asked BEFORE render_begins; the render's own terms (the general path, no live list, boxes
    // wanted, no list buffer re-allocated in this call) stay in render_impl.
    bool prep_stands(const SourceStamps &src, int64_t S, bool option_on) const {
        return option_on && rec.of(src) && rec.last_S == S && lists.lists_gen == src.gen && lists.binning_of(S);
    }

    // ---- events: the only writers ----
    // cel_images_set_nelec: the partials were formed against the old pixels, the resident split was drawn from them
    void new_pixels() { model.partials_gen = 0; split.drop(); nelec_u16 = false; }
    void pixel_range(bool u16) { nelec_u16 = u16; }
    // cel_images_device_ptrs: the caller may write the pixels at any time
    void pixels_handed_out() { nelec_u16 = false; nelec_shared = true; model.partials_gen = 0; }
    // cel_images_set_epsilon: the image was rendered with the old sky level, the partials against it
    void new_sky_level() { model.lambda_gen = 0; model.partials_gen = 0; }
    // cel_images_set_window (another window than before): boxes are cut to the window, and the resident split's patches are
    // boxes of the old one
    void new_window() { rec.recs_gen = rec.hbox_gen = rec.comps_gen = 0; model.lambda_gen = lists.lists_gen = 0; lists.binned_S = -1; split.drop(); }
    void records_regrown() { rec.recs_gen = rec.hbox_gen = rec.comps_gen = 0; lists.binned_S = -1; }
    // k_prep ran on S sources; gen = 0: a partial table or one without boxes is nobody's.  Whoever ran it, the table the
    // lists were binned from may be gone (a partial k_prep, one without boxes, one that compared against another step's
    // word): a render asks binning_of BEFORE its own k_prep and vouches again in render_succeeded.  The component cache was built
    // from the records that stood before: whoever wrote, with whatever values, it is of no records now
    void records_written(uint64_t gen, int64_t S) { rec.recs_gen = gen; rec.last_S = S; rec.comps_gen = 0; lists.binned_S = -1; }
    // k_comps ran on the records that stand (a general render that launched no k_prep: prep_stands held)
    void comps_built() { rec.comps_gen = rec.recs_gen; }
    void host_boxes_read(uint64_t gen) { rec.hbox_gen = gen; }
    // the one-launch render of a small star field wrote k_prep's records, no tile lists and no tile durations
    void small_star_render(uint64_t gen, int64_t S, bool stored) {
        rec.recs_gen = gen; rec.last_S = S; rec.comps_gen = 0;
        lists.lists_gen = 0; lists.cost_S = lists.order_S = -1; lists.binned_S = -1;
        if (stored) model.lambda_gen = 0;
    }
    // the general render: before anything is queued, a render that overwrites them vouches for nothing ...
    void render_begins(bool loglik, bool stores) {
        if (loglik) model.partials_gen = 0;
        lists.lists_gen = 0;
        if (stores) model.lambda_gen = 0;
        model.last_dirty = -1;
    }
    // ... once its lists fitted, for the lists; when it stored the image by the general kernel (vouches) for the image, at
    // this threshold and block count; for the partials only when it formed them (a render WITHOUT the log-likelihood vouches
    // for none: those in the buffer may be of another sky level or threshold although the generation is the same)
    void render_succeeded(const SourceStamps &src, int64_t S, bool costs, bool ordered, bool vouches, double render_T, int parts,
                          bool partials, bool incremental) {
        lists.cost_S = costs ? S : -1; lists.order_S = ordered ? S : -1;
        lists.lists_gen = src.gen; lists.binned_S = S;
        if (vouches) {
            model.lambda_gen = src.gen; model.lambda_uid = src.uid; model.lambda_T = render_T; model.lambda_parts = parts;
            model.partials_gen = partials ? src.gen : 0;
        }
        if (incremental) model.last_dirty = -2;
    }
    void render_overflowed() { lists.cost_S = lists.order_S = -1; lists.binned_S = -1; }
    // a list buffer (d_lists, d_clist) was re-allocated; the image set went over to the two-level binning form
    void lists_regrown() { lists.binned_S = -1; }
    void bin_form_changed() { lists.binned_S = -1; }
    // d_partials was written by someone else: a masked set's Poisson pass, the direct split's noise sums, the E-step's sky term
    void partials_overwritten() { model.partials_gen = 0; }
    // cel_photon_split: masses waiting for cel_stamp_mass_end share a scratch slot with it; the recurrence form rewrites
    // the stamp sums, the direct form keeps its noise partials in the render's buffer
    void split_begins(bool hw) {
        split.split_epoch++;
        if (hw) split.massfx_gen = 0; else model.partials_gen = 0;
    }
    // a RESIDENT split laid its patches out: nothing of the old one holds
    void split_laid_out(int64_t S, int64_t total, bool sums_by_kernel) {
        split.samp_S = S; split.samp_total = total;
        split.ssum_valid = sums_by_kernel;
        split.hsum_valid = split.nz_valid = false;
    }
    void split_totals_from_model(bool yes) { split.rate_in_lambda = yes; }
    // the split has run: host_sums -- its sums and offsets lie in the pinned copies; stamp_sums_gen != 0 -- d_massfx is this
    // catalogue's, summed under the per-source drop threshold tail_T
    void split_ends(bool host_sums, uint64_t stamp_sums_gen, double tail_T) {
        if (host_sums) split.hsum_valid = true;
        if (stamp_sums_gen) { split.massfx_gen = stamp_sums_gen; split.massfx_T = tail_T; }
    }
    void split_lists_built() { split.nz_valid = true; }
};
