// The stamp of desi-mcmc_amd/csrc/field_state.h that lets a render skip the binning of a table that did not change, on the CPU: every event
// of FieldState fires once on a state in which it stands, and it must still stand exactly where the table
// leaves it standing.  Built and run by tests/test_prep_bin_host.py with the host compiler and
// -fsanitize=address,undefined; no GPU, no HIP.
//   B  lists.binning_of(S): the tile lists and everything binned with them were built from the (box, kind) table that stands in
//      d_boxes / d_kind -- the binning kernels may return at once when k_prep finds no box or kind to change
#include "field_state.h"

#include <cstdio>
#include <string>

static int failures = 0;
static const int64_t S = 4;
static const double T = 24.0;

struct World {
    SourceStamps cat;
    FieldState f;
};

// a render of catalogue A succeeded: its lists stand for its table
static World rendered() {
    World w;
    const int32_t types[S] = {0, 1, 0, 0};
    w.cat.created();
    w.cat.all_rows_changed(true);
    w.cat.types_known(types, S);
    w.f.render_begins(true, true);
    w.f.records_written(w.cat.gen, S);
    w.f.render_succeeded(w.cat, S, true, true, true, T, 1, true, false);
    return w;
}

static std::string held(const World &w) {
    std::string s;
    if (w.f.lists.binning_of(S)) s += 'B';
    return s;
}

#define AFTER(event, want)                                                                                   \
    do {                                                                                                     \
        World w = rendered();                                                                                \
        w.f.event;                                                                                           \
        const std::string got = held(w);                                                                     \
        if (got != (want)) { fprintf(stderr, "line %d: after %s: \"%s\", the table says \"%s\"\n", __LINE__, #event, got.c_str(), want); failures++; } \
    } while (0)

int main() {
    {
        FieldState f;
        if (f.lists.binning_of(S) || f.lists.binning_of(0)) { fprintf(stderr, "a new image set vouches\n"); failures++; }
        World w = rendered();
        if (held(w) != "B" || w.f.lists.binning_of(S + 1) || w.f.lists.binning_of(0)) { fprintf(stderr, "the starting point\n"); failures++; }
    }
    // what changes neither the (box, kind) table nor anything binned from it
    AFTER(new_pixels(), "B");
    AFTER(pixel_range(true), "B");
    AFTER(pixels_handed_out(), "B");
    AFTER(new_sky_level(), "B");                        // (the sky level enters neither k_prep nor the lists)
    AFTER(host_boxes_read(w.cat.gen), "B");
    AFTER(render_begins(true, true), "B");              // (a render asks before its k_prep; the k_prep's own event clears)
    AFTER(partials_overwritten(), "B");
    AFTER(split_begins(true), "B");
    AFTER(split_begins(false), "B");
    AFTER(split_laid_out(S, 90, true), "B");
    AFTER(split_totals_from_model(true), "B");
    AFTER(split_ends(true, w.cat.gen, 32.0), "B");
    AFTER(split_lists_built(), "B");
    AFTER(mass.begin(w.cat.gen, 0, 8, -1, nullptr, nullptr), "B");
    AFTER(mass.cancel(), "B");
    // what does
    AFTER(new_window(), "");                            // boxes are cut to the window
    AFTER(records_regrown(), "");                       // the table's buffers are new
    AFTER(records_written(0, S), "");                   // a partial k_prep, or one without boxes
    AFTER(records_written(w.cat.gen, S), "");           // ANY k_prep zeroes the cursor words and may rewrite the table under another step number
    AFTER(small_star_render(w.cat.gen, S, true), "");   // wrote the table, binned nothing
    AFTER(small_star_render(w.cat.gen, S, false), "");
    AFTER(render_overflowed(), "");                     // half-built lists
    AFTER(lists_regrown(), "");
    AFTER(bin_form_changed(), "");
    {   // a render vouches for the source count it binned, and only a render does
        World w = rendered();
        w.f.render_begins(false, false);
        w.f.records_written(w.cat.gen, S + 1);
        if (held(w) != "") { fprintf(stderr, "a k_prep alone vouches\n"); failures++; }
        w.f.render_succeeded(w.cat, S + 1, false, false, false, T, 1, false, false);
        if (w.f.lists.binning_of(S) || !w.f.lists.binning_of(S + 1)) { fprintf(stderr, "the render's own source count\n"); failures++; }
    }
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    puts("prep_bin_stamps: ok");
    return 0;
}
