// The predicate of desi-mcmc_amd/csrc/field_state.h that lets a render read the component cache (k_comps.h), on the CPU: every
// event of FieldState and of SourceStamps fires once on a state in which it holds, and it must still hold exactly where the table
//  leaves it holding.  Built and run by tests/test_comp_cache_host.py with the host compiler and
// -fsanitize=address,undefined; no GPU, no HIP.
//   C  rec.comps_of_records(): the cache's rows were built from the records that stand in d_recs now
//   P  prep_stands(cat, S, option on): the render that asks launches no k_prep -- the only render that reads or builds the cache
#include "field_state.h"

#include <cstdio>
#include <string>

static int failures = 0;
static const int64_t S = 4;
static const double T = 24.0;
static const int32_t kTypes[S] = {0, 1, 0, 0};

struct World {
    SourceStamps cat;
    FieldState f;
};

// what render_impl fires for a general render of `cat`: one that launches k_prep fires records_written; one that does not builds
// the cache when it is not of the records that stand (cache: the option is on and the plan is the cached kernel's)
static void render(World &w, const SourceStamps &cat, int64_t n, bool cache = true) {
    const bool stands = w.f.prep_stands(cat, n, true);
    w.f.render_begins(true, true);
    if (!stands) w.f.records_written(cat.gen, n);
    else if (cache && !w.f.rec.comps_of_records()) w.f.comps_built();
    w.f.render_succeeded(cat, n, true, true, true, T, 1, true, false);
}

// catalogue A rendered twice: the first render prepared, the second built the cache
static World cached() {
    World w;
    w.cat.created();
    w.cat.all_rows_changed(true);
    w.cat.types_known(kTypes, S);
    render(w, w.cat, S);
    render(w, w.cat, S);
    return w;
}

static std::string held(const World &w) {
    std::string s;
    if (w.f.rec.comps_of_records()) s += 'C';
    if (w.f.prep_stands(w.cat, S, true)) s += 'P';
    return s;
}

static void expect(int line, const char *what, const std::string &got, const char *want) {
    if (got != want) { fprintf(stderr, "line %d: after %s: \"%s\", the table says \"%s\"\n", line, what, got.c_str(), want); failures++; }
}

#define AFTER(event, want)                    \
    do {                                      \
        World w = cached();                   \
        w.f.event;                            \
        expect(__LINE__, #event, held(w), want); \
    } while (0)
#define AFTER_CAT(event, want)                \
    do {                                      \
        World w = cached();                   \
        w.cat.event;                          \
        expect(__LINE__, #event, held(w), want); \
    } while (0)

int main() {
    {
        FieldState f;
        if (f.rec.comps_of_records()) { fprintf(stderr, "a new image set vouches for a cache\n"); failures++; }
        World w;
        w.cat.created();
        w.cat.all_rows_changed(true);
        render(w, w.cat, S);
        expect(__LINE__, "the first render (it prepared: the plain kernel, no cache)", held(w), "P");
        render(w, w.cat, S);
        expect(__LINE__, "the second render (it built the cache)", held(w), "CP");
        const uint64_t built = w.f.rec.comps_gen;
        render(w, w.cat, S);
        expect(__LINE__, "the third render", held(w), "CP");
        if (w.f.rec.comps_gen != built || built != w.cat.gen) { fprintf(stderr, "the stamp is the generation of the records it was built from\n"); failures++; }
        // comps_built on records of nobody vouches for nothing
        FieldState g;
        g.comps_built();
        if (g.rec.comps_of_records()) { fprintf(stderr, "a cache of nobody's records\n"); failures++; }
    }
    // what rewrites or disowns the records disowns the cache
    AFTER(records_written(0, S), "");                   // a partial k_prep, or one without boxes
    AFTER(records_written(w.cat.gen, S), "");           // a k_prep of the SAME generation outside a render: whoever wrote, with whatever values
    AFTER(small_star_render(w.cat.gen, S, true), "");
    AFTER(small_star_render(w.cat.gen, S, false), "");
    AFTER(new_window(), "");
    AFTER(records_regrown(), "");
    // what leaves the records alone leaves the cache alone -- whether or not the next render may skip its k_prep
    AFTER(new_pixels(), "CP");
    AFTER(pixel_range(true), "CP");
    AFTER(pixels_handed_out(), "CP");
    AFTER(new_sky_level(), "CP");                       // no sky level is in a row
    AFTER(host_boxes_read(w.cat.gen), "CP");
    AFTER(partials_overwritten(), "CP");
    AFTER(split_begins(true), "CP");
    AFTER(split_begins(false), "CP");
    AFTER(split_laid_out(S, 90, true), "CP");
    AFTER(split_totals_from_model(true), "CP");
    AFTER(split_ends(true, w.cat.gen, 32.0), "CP");
    AFTER(split_lists_built(), "CP");
    AFTER(mass.begin(w.cat.gen, 0, 8, -1, nullptr, nullptr), "CP");
    AFTER(mass.cancel(), "CP");
    AFTER(comps_built(), "CP");
    AFTER_CAT(types_known(kTypes, S), "CP");
    // the lists fall, the records stand: the next render prepares (and disowns the cache THEN: records_written)
    AFTER(render_begins(true, true), "C");
    AFTER(render_begins(false, false), "C");
    AFTER(render_overflowed(), "C");
    AFTER(lists_regrown(), "C");
    AFTER(bin_form_changed(), "C");
    // a new catalogue generation: the records in d_recs are still the ones the cache was built from, nobody may skip k_prep
    AFTER_CAT(all_rows_changed(false), "C");
    AFTER_CAT(all_rows_changed(true), "C");
    {
        const int32_t idx[1] = {2}, type[1] = {0};
        AFTER_CAT(rows_replaced(S, 1, idx, type), "C");
    }
    {   // ... and the render of that generation prepares: plain, the cache stale; the one after it builds
        World w = cached();
        w.cat.all_rows_changed(true);                   // cel_sources_set with identical values
        render(w, w.cat, S);
        expect(__LINE__, "the render of a new generation", held(w), "P");
        render(w, w.cat, S);
        expect(__LINE__, "the render after it", held(w), "CP");
    }
    {   // a list-buffer overflow retry: the render prepared, its retry binned again; the next render builds
        World w = cached();
        w.cat.all_rows_changed(false);
        w.f.render_begins(true, true);
        w.f.records_written(w.cat.gen, S);
        w.f.render_overflowed();
        w.f.lists_regrown();
        w.f.render_succeeded(w.cat, S, true, true, true, T, 1, true, false);
        expect(__LINE__, "an overflow and its retry", held(w), "P");
        render(w, w.cat, S);
        expect(__LINE__, "the render after the retry", held(w), "CP");
    }
    {   // another catalogue object rendered into the set and back: each render of the other one's records prepares
        World w = cached();
        SourceStamps other;
        other.created();
        other.all_rows_changed(true);
        render(w, other, S);
        expect(__LINE__, "another object's render", held(w), "");
        render(w, other, S);
        if (!w.f.rec.comps_of_records() || w.f.rec.comps_gen != other.gen) { fprintf(stderr, "the other object's cache\n"); failures++; }
        render(w, w.cat, S);
        expect(__LINE__, "the first object's render", held(w), "P");
        render(w, w.cat, S);
        expect(__LINE__, "the first object's second render", held(w), "CP");
    }
    {   // stamps are per image set: a second set rendered from the same catalogue changes nothing here, and builds its own
        World w = cached();
        World second;
        second.cat = w.cat;
        render(second, second.cat, S);
        expect(__LINE__, "a second image set's first render", held(second), "P");
        expect(__LINE__, "the first set meanwhile", held(w), "CP");
        render(second, second.cat, S);
        expect(__LINE__, "a second image set's second render", held(second), "CP");
    }
    {   // the option off: renders that skip k_prep build nothing and vouch for nothing; on again: the next one builds
        World w;
        w.cat.created();
        w.cat.all_rows_changed(true);
        render(w, w.cat, S, false);
        render(w, w.cat, S, false);
        expect(__LINE__, "two renders with the option off", held(w), "P");
        render(w, w.cat, S, true);
        expect(__LINE__, "the option on", held(w), "CP");
        render(w, w.cat, S, false);
        expect(__LINE__, "off again: the rows stand, unread", held(w), "CP");
    }
    {   // another source count re-allocates the records
        World w = cached();
        SourceStamps big;
        big.created();
        big.all_rows_changed(true);
        w.f.records_regrown();
        render(w, big, 2 * S);
        if (w.f.rec.comps_of_records()) { fprintf(stderr, "a cache across a re-allocation\n"); failures++; }
        render(w, big, 2 * S);
        if (!w.f.rec.comps_of_records() || !w.f.prep_stands(big, 2 * S, true)) { fprintf(stderr, "the larger catalogue's cache\n"); failures++; }
    }
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    puts("comp_cache_stamps: ok");
    return 0;
}
