// The event table of desi-mcmc_amd/csrc/field_state.h, row by row, on the CPU: every product is set "vouched for catalogue A",
// one event fires, and exactly the predicates the table leaves standing must still hold.  Built and run by
// tests/test_abi_and_host.py with the host compiler and -fsanitize=address,undefined; no GPU, no HIP.
#include "field_state.h"

#include <cstdio>
#include <cstdlib>
#include <string>

static int failures = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } \
    } while (0)

static const int64_t S = 4;
static const double T = 24.0, TS = 32.0;     // the field render's drop threshold and the per-source kernels'
static const int todo_list[1] = {0};
static double mass_values[8];

struct World {
    SourceStamps was, now;      // catalogue A as the products saw it, and A with one row replaced since
    FieldState f;
};

// every product vouched for catalogue A, then one row of A replaced from the host (what the dirty-tile render starts from)
static World vouched() {
    World w;
    const int32_t types[S] = {0, 1, 0, 0};
    w.now.created();
    w.now.all_rows_changed(true);
    w.now.types_known(types, S);
    FieldState &f = w.f;
    f.pixel_range(true);
    f.render_begins(true, true);
    f.records_written(w.now.gen, S);
    f.render_succeeded(w.now, S, true, true, true, T, 1, true, false);
    f.host_boxes_read(w.now.gen);
    f.split_begins(true);
    f.split_laid_out(S, 100, true);
    f.split_totals_from_model(false);
    f.split_ends(true, w.now.gen, TS);
    f.split_lists_built();
    f.mass.begin(w.now.gen, f.split.split_epoch, S * 2, S, todo_list, mass_values);
    w.was = w.now;
    const int32_t idx[1] = {2}, type[1] = {0};
    w.now.rows_replaced(S, 1, idx, type);
    return w;
}

// one letter per predicate that holds:  r records  b host boxes  l lists  o launch order  c tile costs  m model image  p partials
// t totals from the model image  i dirty-tile render with a log-likelihood  j ... without  s resident split of S  u device sums
// h host sums  z photon lists  x stamp sums  q pending mass intact  6 16-bit pixel range
static std::string held(const World &w) {
    const FieldState &f = w.f;
    std::string s;
    if (f.rec.of(w.was)) s += 'r';
    if (f.rec.host_boxes_of(w.was)) s += 'b';
    if (f.lists.lists_gen == w.was.gen) s += 'l';
    if (f.lists.order_ready(S)) s += 'o';
    if (f.lists.costs_of(S)) s += 'c';
    if (f.model.lambda_gen == w.was.gen) s += 'm';
    if (f.model.partials_gen == w.was.gen) s += 'p';
    if (f.model_current(w.was, T)) s += 't';
    if (f.incremental_base(w.now, S, T, true)) s += 'i';
    if (f.incremental_base(w.now, S, T, false)) s += 'j';
    if (f.split.resident_of(S)) s += 's';
    if (f.split.ssum_valid) s += 'u';
    if (f.split.hsum_valid) s += 'h';
    if (f.split.nz_valid) s += 'z';
    if (f.split.sums_of(w.was, TS)) s += 'x';
    if (f.mass.pending >= 0 && f.mass.intact(f.rec, f.split)) s += 'q';
    if (f.nelec_u16) s += '6';
    return s;
}

#define AFTER(event, want)                                                                                   \
    do {                                                                                                     \
        World w = vouched();                                                                                 \
        w.f.event;                                                                                           \
        const std::string got = held(w);                                                                     \
        if (got != (want)) { fprintf(stderr, "line %d: after %s: \"%s\", the table says \"%s\"\n", __LINE__, #event, got.c_str(), want); failures++; } \
    } while (0)

static void catalogue_functions() {
    SourceStamps a, b;
    a.created(); b.created();
    CHECK(a.uid != 0 && b.uid > a.uid && a.gen == 0 && a.n_gal == -1);
    const int32_t types[S] = {0, 1, 2, 0};
    a.all_rows_changed(true);
    CHECK(a.gen > b.uid && a.full_gen == a.gen && a.row_gen.empty() && a.n_gal == -1 && a.h_type.empty());
    a.types_known(types, S);
    CHECK(a.n_gal == 2 && a.h_type.size() == (size_t)S && a.h_type[2] == 2);
    // rows replaced from the host: the count stays exact, the rows carry the new generation, full_gen stays
    const uint64_t g0 = a.gen;
    const int32_t idx[2] = {1, 3}, type[2] = {0, 1};
    a.rows_replaced(S, 2, idx, type);
    CHECK(a.gen > g0 && a.full_gen == g0 && a.n_gal == 2 && a.h_type[1] == 0 && a.h_type[3] == 1);
    CHECK(a.row_gen.size() == (size_t)S && a.row_gen[0] == 0 && a.row_gen[1] == a.gen && a.row_gen[2] == 0 && a.row_gen[3] == a.gen);
    const int32_t idx1[1] = {1}, type1[1] = {0};
    const uint64_t g1 = a.gen;
    a.rows_replaced(S, 1, idx1, type1);
    CHECK(a.n_gal == 2 && a.row_gen[1] == a.gen && a.row_gen[3] == g1 && a.gen > g1);
    // a device sampler that leaves the types alone: no row stamps, the types and their count stay
    a.all_rows_changed(false);
    CHECK(a.full_gen == a.gen && a.row_gen.empty() && a.n_gal == 2 && a.h_type.size() == (size_t)S);
    // ... one that writes them: unknown until they are read back
    a.all_rows_changed(true);
    CHECK(a.n_gal == -1 && a.h_type.empty() && a.row_gen.empty());
    a.rows_replaced(S, 1, idx1, type1);             // (without the host's types the count cannot be kept)
    CHECK(a.n_gal == -1 && a.h_type.empty() && a.row_gen.size() == (size_t)S);
    const int32_t stars[S] = {0, 0, 0, 0};
    a.types_known(stars, S);
    CHECK(a.n_gal == 0 && a.h_type.size() == (size_t)S);
    // a catalogue of no rows; clearing an empty row_gen changes nothing
    b.all_rows_changed(true);
    b.types_known(stars, 0);
    CHECK(b.n_gal == 0 && b.h_type.empty() && b.row_gen.empty() && b.gen > a.gen);
}

int main() {
    catalogue_functions();
    {   // the starting point: everything holds
        World w = vouched();
        CHECK(held(w) == "rblocmptijsuhzxq6");
        CHECK(!w.f.nelec_shared && w.f.model.last_dirty == -1 && w.f.rec.last_S == S);
    }
    AFTER(new_pixels(), "rblocmtjq");
    AFTER(pixels_handed_out(), "rblocmtjsuhzxq");
    AFTER(new_sky_level(), "rblocsuhzxq6");
    AFTER(new_window(), "ocp6");                                    // (the resident split's patches are boxes of the old window)
    AFTER(records_regrown(), "locmpsuhzx6");
    AFTER(records_written(0, S), "locmpsuhzx6");                    // a partial table, or one without boxes
    AFTER(records_written(w.was.gen, S), "rblocmptijsuhzxq6");      // the same catalogue again
    AFTER(records_written(w.now.gen, S), "locmpsuhzx6");            // another generation
    AFTER(records_written(w.was.gen, S + 1), "rblocmptsuhzxq6");    // (last_S: the dirty-tile render's source count)
    AFTER(small_star_render(w.was.gen, S, true), "rbpsuhzxq6");
    AFTER(small_star_render(w.was.gen, S, false), "rbmpsuhzxq6");
    AFTER(render_begins(true, true), "rbocsuhzxq6");
    AFTER(render_begins(false, true), "rbocpsuhzxq6");
    AFTER(render_begins(true, false), "rbocmsuhzxq6");
    AFTER(render_begins(false, false), "rbocmpsuhzxq6");
    AFTER(render_overflowed(), "rblmptijsuhzxq6");
    AFTER(partials_overwritten(), "rblocmtjsuhzxq6");
    AFTER(split_begins(true), "rblocmptijsuhz6");
    AFTER(split_begins(false), "rblocmtjsuhzx6");
    AFTER(split_laid_out(S, 90, true), "rblocmptijsuxq6");
    AFTER(split_laid_out(S, 90, false), "rblocmptijsxq6");
    AFTER(split_laid_out(S + 1, 90, true), "rblocmptijuxq6");
    AFTER(split_ends(false, 0, 8.0), "rblocmptijsuhzxq6");          // (no stamp sums made: those that lie there keep their threshold)
    {   // a render of the catalogue as it is now: what it vouches for depends on what it did
        World w = vouched();
        w.f.render_begins(true, true);
        w.f.records_written(w.now.gen, S);
        CHECK(w.f.model.last_dirty == -1);
        w.f.render_succeeded(w.now, S, true, false, true, T, 1, true, true);
        w.was = w.now;
        CHECK(held(w) == "rlcmptsuhz6" && w.f.model.last_dirty == -2);      // (no host boxes, no order, stamp sums and masses of the old generation)
        w.f.render_begins(false, true);
        w.f.render_succeeded(w.now, S, false, false, true, T, 1, false, false);
        CHECK(held(w) == "rlmtsuhz6");                  // without the log-likelihood: no partials
        w.f.render_begins(true, false);
        w.f.render_succeeded(w.now, S, true, true, false, T, 1, true, false);
        CHECK(held(w) == "rlocmtsuhz6");                // an image of the caller's own, a strict one, NO_STORE: the lists only
        w.f.render_begins(true, true);
        w.f.render_succeeded(w.now, S, true, true, true, T, 2, true, false);
        CHECK(held(w) == "rlocmptsuhz6");
        const int32_t idx[1] = {0}, type[1] = {0};
        w.now.rows_replaced(S, 1, idx, type);
        CHECK(!w.f.incremental_base(w.now, S, T, false));                  // two blocks per tile: no base for the dirty-tile render
        w.f.render_begins(true, true);
        w.f.records_written(w.now.gen, S);
        w.f.render_succeeded(w.now, S, true, true, true, T, 1, true, false);
        w.now.rows_replaced(S, 1, idx, type);
        CHECK(w.f.incremental_base(w.now, S, T, true));
        CHECK(!w.f.incremental_base(w.now, S, 32.0, true));                // another drop threshold
        SourceStamps other = w.now;
        other.created();
        CHECK(!w.f.incremental_base(other, S, T, true));                   // another object with the same generations
        w.now.all_rows_changed(false);
        CHECK(!w.f.incremental_base(w.now, S, T, true));                   // a device sampler rewrote every row since
    }
    {   // the split's ends, and the pending masses: handed out once
        World w = vouched();
        w.f.split_begins(true);
        w.f.split_laid_out(S, 80, true);
        CHECK(held(w) == "rblocmptijsu6");
        w.f.split_ends(true, w.was.gen, TS);
        CHECK(held(w) == "rblocmptijsuhx6");
        w.f.split_lists_built();
        CHECK(held(w) == "rblocmptijsuhzx6");
        w.f.split_totals_from_model(true);
        CHECK(w.f.split.rate_in_lambda);
        int64_t n = -5, todo = -5;
        CHECK(w.f.mass.take(&n, &todo) && n == 2 * S && todo == S && w.f.mass.todo_ptr == todo_list && w.f.mass.values == mass_values);
        CHECK(!w.f.mass.take(&n, &todo) && w.f.mass.pending == -1 && w.f.mass.todo_S == -1);
        w.f.mass.begin(w.was.gen, w.f.split.split_epoch, 0, -1, nullptr, nullptr);
        CHECK(w.f.mass.take(&n, &todo) && n == 0 && todo == -1);
        w.f.mass.begin(w.was.gen, w.f.split.split_epoch, 8, -1, nullptr, mass_values);
        w.f.mass.cancel();
        CHECK(!w.f.mass.take(&n, &todo));
    }
    {   // the thresholds the products were made at: a reader at another one is not served
        World w = vouched();
        CHECK(w.f.model_current(w.was, T) && !w.f.model_current(w.was, TS) && !w.f.model_current(w.was, 8.0));   // the split's totals
        CHECK(w.f.split.sums_of(w.was, TS) && !w.f.split.sums_of(w.was, T) && !w.f.split.sums_of(w.was, 8.0));   // the mass short cut
        CHECK(!w.f.split.sums_of(w.now, TS));                              // (and never another generation's)
        w.f.split_begins(true);
        w.f.split_laid_out(S, 100, true);
        w.f.split_ends(true, w.was.gen, 8.0);                              // a split under a coarse per-source threshold ...
        CHECK(w.f.split.sums_of(w.was, 8.0) && !w.f.split.sums_of(w.was, TS));     // ... vouches for masses at that one alone
        CHECK(w.f.model_current(w.was, T));                                // (the field render's threshold is not the split's business)
    }
    {   // a new window behind a pending cel_stamp_mass_begin: the records it summed are nobody's, _end refuses
        World w = vouched();
        w.f.new_window();
        CHECK(w.f.mass.pending >= 0 && !w.f.mass.intact(w.f.rec, w.f.split));
        CHECK(w.f.split.samp_S == 0 && w.f.split.samp_total == 0 && !w.f.split.resident_of(S));
    }
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    puts("field_state: ok");
    return 0;
}
