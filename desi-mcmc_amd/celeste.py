"""Drop-in mirror of the render + likelihood API of CelestePy/celeste.py (reference lines cited
per function).  Same names, argument order and return tuples; the arithmetic runs in the HIP
kernels behind the C ABI (include/celeste_hip.h).  No CPU fallback exists: without the built
library and a GPU these functions raise.

Divergences from the reference, all documented in DESIGN.md "Quirks":
  Q1  a star that fails the reference's overlap test contributes nothing to gen_model_image
      (the reference multiplies None and raises TypeError);
  Q3  galaxies are accepted by gen_model_image / celeste_likelihood: each source's own patch is
      accumulated (the reference's gen_galaxy_psf_image ignores return_patch and breaks there);
  planck  stars given by temperature (`src.t`) need a hook: set `photons_expected_brightness`.
"""
import collections
import warnings
import os
import itertools
import operator
import sys
import weakref

import numpy as np

from . import field as _field
from .fits_image import FitsImage  # noqa: F401  (re-exported like the reference does)

BANDS = np.array(['u', 'g', 'r', 'i', 'z'], dtype=object)

#: optional hook with the signature of planck.photons_expected_brightness(t, b, band)
#: (CelestePy/planck.py:155); black-body photometry itself is outside this path.
photons_expected_brightness = None

_DEVICE = 0


def set_device(device):
    global _DEVICE
    _DEVICE = int(device)
    for key in list(_SETS):
        _evict(key)


# ---- device-resident image sets, cached per python image object ---------------------------
# One ImageSet (nelec + model image + split totals on the device: 24 bytes per pixel) per distinct
# tuple of image objects, least-recently-used first.  Entries are evicted -- and their device
# memory released at once, not at garbage collection -- when the cache holds more than
# CACHE_MAX_BYTES or CACHE_MAX_SETS, or when one of their images has been collected.
# Callers that touch only SOME images of a set that is already resident (a source sampled in 3
# of a field's 5 bands) are handed that set and the positions of their images in it
# (_image_subset) instead of a second copy of the same pixels.
CACHE_MAX_BYTES = 16 << 30
CACHE_MAX_SETS = 64
_SETS = collections.OrderedDict()      # key: tuple of id(image) -> [refs, ImageSet, eps list, bytes]


def _set_bytes(images):
    return sum(24 * im.nelec.size for im in images)


def _evict(key):
    ent = _SETS.pop(key, None)
    if ent is not None:
        ent[1].close()                 # cel_images_destroy now


def _in_use(ent):
    """someone outside the cache holds the ImageSet (a ModelGibbs over these images, a caller in the
    middle of a call): closing it under them would turn their next call into an error"""
    return sys.getrefcount(ent[1]) > 2          # the entry's list + getrefcount's argument


def _cache_trim(keep=None):
    for key in [k for k, e in _SETS.items() if any(r() is None for r in e[0])]:
        _evict(key)
    over = lambda: len(_SETS) > CACHE_MAX_SETS or sum(e[3] for e in _SETS.values()) > CACHE_MAX_BYTES   # noqa: E731
    for key in list(_SETS):                      # least recently used first
        if not over():
            break
        if key == keep or _in_use(_SETS[key]):
            continue
        _evict(key)


def _sync_epsilon(ent, images):
    iset = ent[1]
    for b, im in enumerate(images):          # epsilon is resampled by Gibbs (models.py:156-160)
        if im.epsilon != iset.eps[b]:        # iset.eps mirrors what the device holds, whoever set it
            iset.set_epsilon(b, im.epsilon)


def _image_set(images):
    """ImageSet for a tuple of same-shape FitsImage objects (uploaded once, nelec is immutable)."""
    images = tuple(images)
    key = tuple(id(im) for im in images)
    hit = _SETS.get(key)
    if hit is not None and all(r() is im for r, im in zip(hit[0], images)):
        _SETS.move_to_end(key)
        _sync_epsilon(hit, images)
        return hit[1]
    if hit is not None:
        _evict(key)                          # ids re-used by other objects
    H, W = images[0].nelec.shape
    ctx = _field.default_context(_DEVICE)
    bands = np.stack([im.band_record() for im in images])
    # (`observed`: nelec, with NaN at the invvar == 0 pixels of an image built with mask_invvar=True)
    iset = _field.ImageSet(ctx, bands, H, W, nelec=np.stack([getattr(im, "observed", im.nelec) for im in images]))
    try:
        refs = [weakref.ref(im) for im in images]
    except TypeError:
        return iset
    _SETS[key] = [refs, iset, [im.epsilon for im in images], _set_bytes(images)]
    _cache_trim(keep=key)
    return iset


def _image_subset(images):
    """-> (ImageSet, positions): a resident set that CONTAINS `images` and where each sits in it;
    a new set of exactly `images` when there is none."""
    images = tuple(images)
    want = [id(im) for im in images]
    for key in reversed(_SETS):
        if set(want) <= set(key):
            ent = _SETS[key]
            pos = [key.index(i) for i in want]
            if all(ent[0][p]() is im for p, im in zip(pos, images)):
                _SETS.move_to_end(key)
                live = [r() for r in ent[0]]
                if all(im is not None for im in live):
                    _sync_epsilon(ent, live)
                    return ent[1], pos
    return _image_set(images), list(range(len(images)))


def _flux(src, band):
    f = src.fluxes
    if isinstance(f, dict):
        return f[band]
    return f[list(BANDS).index(band)]


def expected_photons(src, image):
    """The multiplier of gen_src_image: three flux conventions (celeste.py:35-62)."""
    if src.a == 0:
        if src.t:
            if photons_expected_brightness is None:
                raise NotImplementedError("star given by temperature: set celeste.photons_expected_brightness "
                                          "to a planck.photons_expected_brightness(t, b, band) callable")
            return photons_expected_brightness(src.t, src.b, image.band)
        return image.nmgy2counts(_flux(src, image.band))
    elif src.a == 1:
        return image.nmgy2counts(_flux(src, image.band))
    elif src.a is None and src.fluxes is not None:
        return image.kappa * _flux(src, image.band)
    raise Exception("No way to compute expected photons without at least fluxes or brightness")


def _gather_fluxes(srcs, images, bidx, fls=None):
    """(S, B) fluxes in the images' bands: one C-level pass over the sources (itemgetter + fromiter: a nest of Python
    subscripts cost 8x as much at 10 000 sources), not S x B calls"""
    S = len(srcs)
    if fls is None:
        fls = [s.fluxes for s in srcs]
    kinds = set(map(type, fls))
    if kinds == {dict}:
        names = [im.band for im in images]
        if len(names) == 1:
            return np.fromiter(map(operator.itemgetter(names[0]), fls), dtype=np.float64, count=S).reshape(S, 1)
        return np.fromiter(itertools.chain.from_iterable(map(operator.itemgetter(*names), fls)), dtype=np.float64,
                           count=S * len(names)).reshape(S, len(names))
    if dict not in kinds:
        if kinds == {np.ndarray}:
            return np.concatenate(fls).astype(np.float64, copy=False).reshape(S, -1)[:, bidx]
        return np.array(fls, dtype=np.float64).reshape(S, -1)[:, bidx]
    return np.array([[_flux(s, im.band) for im in images] for s in srcs], dtype=np.float64).reshape(S, len(images))


def _catalogue_rows(srcs):
    """-> (SrcCatalog, row indices or None = every row in order) when `srcs` is a list of views of ONE catalogue
    (SrcCatalog.views() or any selection of it); None otherwise.  The full list is recognised by object identity
    in one C-level pass; a selection costs one attribute read per source."""
    from .celeste_src import _SrcView
    if not isinstance(srcs, (list, tuple)) or not srcs or type(srcs[0]) is not _SrcView:
        return None
    cat = srcs[0]._c
    whole = getattr(cat, "_views", None)
    if whole is not None and len(srcs) == len(whole) and (srcs is whole or all(map(operator.is_, srcs, whole))):
        return cat, None
    if not all(type(s) is _SrcView and s._c is cat for s in srcs):
        return None
    return cat, np.fromiter(map(operator.attrgetter("_i"), srcs), dtype=np.int64, count=len(srcs))


def _source_arrays(srcs, images, counts_fn=expected_photons):
    """(type[S], radec[S,2], counts[S,B], shape[S,4]) of a sequence of SrcParams for the device.
    A SrcCatalog -- or a list of its views, SrcCatalog.views() -- hands its arrays over without any per-source
    work; a plain list of SrcParams is gathered with one C-level pass per attribute (no S x B nest of Python
    calls) when every source takes the same flux convention, and source by source otherwise."""
    from .celeste_src import SrcCatalog
    B = len(images)
    bidx = [list(BANDS).index(im.band) for im in images]
    calib = np.array([im.calib for im in images])
    kappa = np.array([im.kappa for im in images])
    rows = None
    if not isinstance(srcs, SrcCatalog):
        hit = _catalogue_rows(srcs)
        if hit is not None:
            srcs, rows = hit
    if isinstance(srcs, SrcCatalog):
        a, u, fl5, sh = srcs.a, srcs.u, srcs.fluxes, srcs.shape
        if rows is not None:
            a, u, fl5, sh = a[rows], u[rows], fl5[rows], sh[rows]
        fl = fl5[:, bidx]
        if counts_fn is expected_photons:
            # celeste.py:35-62: stars / galaxies flux / calib * kappa, untyped rows kappa * flux
            counts = np.where((a >= 0)[:, None], fl / calib[None, :] * kappa[None, :], kappa[None, :] * fl)
        else:
            counts = (fl / calib[None, :]) * kappa[None, :]          # flux_dict convention (celeste.py:80-81,94)
        typ = (a == 1).astype(np.int32)
        return typ, u, counts, np.where((a == 1)[:, None], sh, 0.0)
    if type(srcs) is list and len(srcs) >= _LIST_CACHE_MIN and _LIST_CACHE_MODE[0] != "off":
        if _LIST_CACHE_MODE[0] == "exact":
            return _diffed_list_arrays(srcs, images, counts_fn, bidx, calib, kappa)
        return _cached_list_arrays(srcs, images, counts_fn, bidx, calib, kappa)
    return _gather_plain(srcs, images, counts_fn, bidx, calib, kappa)


def _attr_column(srcs, name, S):
    """one attribute of every source as an object array: a single C-level pass"""
    return np.fromiter(map(operator.attrgetter(name), srcs), dtype=object, count=S)


_NATIVE = [None, None]       # the C-level gather (desi-mcmc_amd/csrc_host/srcgather.c): module (False: not built) and SrcParams' slot offsets


def _native_gather():
    if _NATIVE[0] is None:
        try:
            from . import _srcgather
            from .celeste_src import SrcParams
            _NATIVE[1] = (SrcParams, _srcgather.slot_offsets(SrcParams, ("a", "u", "t", "theta", "sigma", "phi", "rho", "fluxes")))
            _NATIVE[0] = _srcgather
        except Exception:                          # not built: numpy's passes below do the same, 10 x slower
            _NATIVE[0] = False
    return _NATIVE[0]


def _gather_plain(srcs, images, counts_fn, bidx, calib, kappa):
    """the arrays of a plain sequence of SrcParams.  A list of plain SrcParams objects (stars and galaxies by flux, locations and
    fluxes in float64 arrays or band-letter dicts) is read in ONE C-level pass over the objects' slots (csrc_host/srcgather.c:
    0.3 ms at 10 000 sources); anything else by one numpy pass per attribute when every source takes the same flux convention,
    source by source otherwise.  The three routes return the same bits."""
    B = len(images)
    S = len(srcs)
    g = _native_gather() if (type(srcs) is list and S) else None
    if g:
        typ = np.empty(S, dtype=np.int32)
        radec, fl, shape, untyped = np.empty((S, 2)), np.empty((S, B)), np.empty((S, 4)), np.empty(S, dtype=bool)
        cls, offs = _NATIVE[1]
        if g.gather(srcs, cls, offs, tuple(im.band for im in images), tuple(int(i) for i in bidx), typ, radec, fl, shape, untyped) == S:
            if counts_fn is expected_photons:
                counts = np.where(untyped[:, None], kappa[None, :] * fl, fl / calib[None, :] * kappa[None, :])
            else:
                counts = (fl / calib[None, :]) * kappa[None, :]
            return typ, radec, counts, shape
    radec = np.zeros((S, 2))
    shape = np.zeros((S, 4))
    counts = np.zeros((S, B))
    # what decides the route: type, temperature, flux container
    a_col = _attr_column(srcs, "a", S)
    f_col = _attr_column(srcs, "fluxes", S)
    try:
        t_col = _attr_column(srcs, "t", S)
    except AttributeError:                      # records without a temperature attribute
        t_col = np.array([getattr(s, "t", None) for s in srcs], dtype=object)
    typ = (a_col == 1).astype(np.int32)
    simple = counts_fn is not expected_photons or not any(t_col.tolist())
    if S and simple:
        us = list(map(operator.attrgetter("u"), srcs))
        if set(map(type, us)) == {np.ndarray} and us[0].shape == (2,):
            radec[:] = np.concatenate(us).reshape(S, 2)         # a (3,) among them fails the reshape, as np.array would
        else:
            radec[:] = np.array(us, dtype=np.float64).reshape(S, 2)
        gal = np.nonzero(typ)[0]
        if gal.size:
            pick = srcs if gal.size == S else [srcs[i] for i in gal]
            shape[gal] = np.fromiter(itertools.chain.from_iterable(map(operator.attrgetter("theta", "sigma", "phi", "rho"), pick)),
                                     dtype=np.float64, count=4 * gal.size).reshape(gal.size, 4)
        fls = f_col.tolist()
        if counts_fn is expected_photons:
            untyped = np.equal(a_col, None)
            if any(f is None for f, u_ in zip(fls, untyped.tolist()) if u_):
                raise Exception("No way to compute expected photons without at least fluxes or brightness")
            fl = _gather_fluxes(srcs, images, bidx, fls)
            counts = np.where(untyped[:, None], kappa[None, :] * fl, fl / calib[None, :] * kappa[None, :])
        else:
            fl = _gather_fluxes(srcs, images, bidx, fls)      # flux_dict = the same numbers by band letter
            counts = (fl / calib[None, :]) * kappa[None, :]
        return typ, radec, counts, shape
    for s, src in enumerate(srcs):
        radec[s] = src.u
        if src.a == 1:
            shape[s] = [src.theta, src.sigma, src.phi, src.rho]
        for b, im in enumerate(images):
            counts[s, b] = counts_fn(src, im)
    return typ, radec, counts, shape


# ---- a LIST of SrcParams evaluated again and again -------------------------------------------------------------------
# celeste_em.py:25,159, celeste_mcmc.py:130 and every move of util/infer/mcmc_transitions.py:37-152 call
# celeste_likelihood*(list_of_SrcParams, ...) after changing ONE source.  Three ways to read such a list:
#
#   "exact" (the default)  EVERY source is re-read on EVERY call, exactly as the reference does (celeste.py:203-219): whatever
#       was done to the objects -- an assignment, an edit in place (src.u[0] = x, src.fluxes['r'] = f), a changed calibration
#       hook -- the call sees it.  The freshly gathered arrays are compared with the ones the device holds (kept per list
#       object, image group and flux convention) and only the rows that differ go up (cel_sources_set_rows), so a
#       single-source move still takes the incremental render.  Nothing is ever answered from host-side state.
#   "stamps" (opt-in, the fast mode)  the arrays are gathered once; afterwards only the objects whose modification stamp moved
#       (celeste_src.SrcParams.__setattr__) are read again: one C-level identity pass instead of a gather, 3.7 ms less per call
#       at 10 000 sources.  A container changed IN PLACE without an attribute assignment afterwards moves no stamp and is
#       NOT seen until celeste_src.touch(src) (the reference's own moves assign, mcmc_transitions.py:49-51); a rotating audit
#       (a sixteenth of the list re-read per call) meets such an edit within 16 calls, warns, and re-reads the whole list.
#   "off"  no host-side state at all: gathered and uploaded whole on every call.
#
# celeste.list_cache(mode) or CEL_LIST_CACHE=<mode> in the environment.  A SrcCatalog (or its views()) needs none of this.
_LIST_CACHE_MIN = 64          # shorter lists are gathered every time (cheaper than the bookkeeping)
_LIST_CACHE_MODES = ("exact", "stamps", "off")
_LIST_CACHE_MODE = [os.environ.get("CEL_LIST_CACHE", "exact")]
if _LIST_CACHE_MODE[0] not in _LIST_CACHE_MODES:
    raise ValueError("CEL_LIST_CACHE=%r: one of %s" % (_LIST_CACHE_MODE[0], ", ".join(_LIST_CACHE_MODES)))
_AUDIT_PARTS = 16


def list_cache(mode=None):
    """how a plain LIST of SrcParams passed again and again is read: "exact" (default) -- every source re-read on every call,
    as the reference does; only the rows that differ from the device's copy are uploaded; "stamps" -- gathered once,
    afterwards only the objects assigned to since (SrcParams.__setattr__ / celeste_src.touch) are re-read, with a rotating
    audit that warns and re-reads everything when it meets an in-place edit nobody stamped; "off" -- no state kept, whole
    upload every call.  -> the mode in force (mode=None only asks)"""
    if mode is not None:
        if mode not in _LIST_CACHE_MODES:
            raise ValueError("list_cache: one of %s" % ", ".join(repr(m) for m in _LIST_CACHE_MODES))
        if mode != _LIST_CACHE_MODE[0]:
            _LIST_CACHE.clear()
            _ENTRY_OF.clear()
        _LIST_CACHE_MODE[0] = mode
    return _LIST_CACHE_MODE[0]

_LIST_CACHE = collections.OrderedDict()   # (id(list), image ids, counts_fn) -> _ListEntry; a handful of lists
_LIST_CACHE_MAX = 4
_ENTRY_OF = {}                # id(typ array) -> entry: how _device_sources recognises cached arrays


class _ListEntry(object):
    __slots__ = ("srcs", "objs", "stamps", "clock", "imgkey", "typ", "radec", "counts", "shape", "version", "log", "audit", "index")

    def rows_since(self, version):
        """rows changed after `version`, or None when the log no longer reaches back that far"""
        if version == self.version:
            return np.zeros(0, dtype=np.int64)
        if not self.log or self.log[0][0] > version + 1:
            return None
        return np.unique(np.concatenate([r for v, r in self.log if v > version]))


def _stamp_column(srcs, S):
    try:
        return np.fromiter(map(operator.attrgetter("_stamp"), srcs), dtype=np.int64, count=S)
    except AttributeError:       # objects that are not SrcParams (no stamps): never cached
        return None


def _cached_list_arrays(srcs, images, counts_fn, bidx, calib, kappa):
    from .celeste_src import clock, stamped_since
    S = len(srcs)
    key = (id(srcs), tuple(map(id, images)), counts_fn, photons_expected_brightness)     # a changed hook is another entry
    imgkey = (tuple(bidx), tuple(calib.tolist()), tuple(kappa.tolist()))
    ent = _LIST_CACHE.get(key)
    if ent is not None and ent.srcs is srcs and len(ent.objs) == S and ent.imgkey == imgkey and all(map(operator.is_, srcs, ent.objs)):
        _LIST_CACHE.move_to_end(key)
        now = clock()
        if now != ent.clock:                   # some SrcParams somewhere was assigned to since the last look
            ids = stamped_since(ent.clock)     # which: from the assignment log's tail, or -- the log too short -- from every stamp
            if ids is not None and len(ids) <= 64 and ent.index is not None:
                rows = np.array(sorted({ent.index[i] for i in ids if i in ent.index}), dtype=np.int64)
                stamps = ent.stamps
                if rows.size:
                    stamps = ent.stamps.copy()
                    stamps[rows] = [srcs[i]._stamp for i in rows]
            else:
                stamps = _stamp_column(srcs, S)
                rows = np.nonzero(stamps != ent.stamps)[0]
            if rows.size > max(S // 8, 16):
                ent = None                      # most of the list moved: gather it whole
            else:
                if rows.size:
                    t, r, c, sh = _gather_plain([srcs[i] for i in rows], images, counts_fn, bidx, calib, kappa)
                    ent.typ[rows], ent.radec[rows], ent.counts[rows], ent.shape[rows] = t, r, c, sh
                    ent.version += 1
                    ent.log.append((ent.version, rows))
                    del ent.log[:-16]
                ent.stamps, ent.clock = stamps, now
        if ent is not None and _audit_rows(ent, srcs, images, counts_fn, bidx, calib, kappa):
            return ent.typ, ent.radec, ent.counts, ent.shape
    now = clock()
    stamps = _stamp_column(srcs, S)
    arrs = _gather_plain(srcs, images, counts_fn, bidx, calib, kappa)
    if stamps is None:
        return arrs
    old = _LIST_CACHE.pop(key, None)
    if old is not None:
        _ENTRY_OF.pop(id(old.typ), None)
    ent = _ListEntry()
    ent.srcs, ent.objs, ent.stamps, ent.clock, ent.imgkey = srcs, list(srcs), stamps, now, imgkey
    ent.typ, ent.radec, ent.counts, ent.shape = arrs
    ent.version, ent.log, ent.audit = 0, [], 0
    ent.index = {i: k for k, i in enumerate(map(id, srcs))}          # id(object) -> row (the entry keeps the objects alive: ids stay theirs)
    if len(ent.index) != S:
        ent.index = None                                             # an object listed twice: the stamps decide
    _LIST_CACHE[key] = ent
    _ENTRY_OF[id(ent.typ)] = ent
    while len(_LIST_CACHE) > _LIST_CACHE_MAX:
        _, gone = _LIST_CACHE.popitem(last=False)
        _ENTRY_OF.pop(id(gone.typ), None)
    return arrs


def _audit_rows(ent, srcs, images, counts_fn, bidx, calib, kappa):
    """re-read the next sixteenth of the list and compare it with the cached rows: an object changed in place without an
    assignment (src.u[0] = x, src.fluxes['r'] = f) makes the cache stale without moving its stamp"""
    S = len(srcs)
    n = min(S, max(64, -(-S // _AUDIT_PARTS)))
    lo = ent.audit if ent.audit + n <= S else max(S - n, 0)
    ent.audit = (lo + n) % S
    t, r, c, sh = _gather_plain(srcs[lo:lo + n], images, counts_fn, bidx, calib, kappa)
    ok = (np.array_equal(t, ent.typ[lo:lo + n]) and np.array_equal(r, ent.radec[lo:lo + n], equal_nan=True) and
          np.array_equal(c, ent.counts[lo:lo + n], equal_nan=True) and np.array_equal(sh, ent.shape[lo:lo + n], equal_nan=True))
    if not ok:
        bad = lo + int(np.nonzero(np.any(r != ent.radec[lo:lo + n], axis=1) | np.any(c != ent.counts[lo:lo + n], axis=1) |
                                  np.any(sh != ent.shape[lo:lo + n], axis=1) | (t != ent.typ[lo:lo + n]))[0][0])
        warnings.warn("celeste.list_cache('stamps'): source %d of this list was changed IN PLACE (src.u[0] = x, src.fluxes['r'] = f) "
                      "without an attribute assignment afterwards, or its counts function is not reproducible; the values returned "
                      "since that edit did not see it.  The whole list is read again now.  Assign the attribute (src.u = u, as the "
                      "reference's moves do), call celeste_src.touch(src), or use the default list_cache('exact')" % bad,
                      RuntimeWarning, stacklevel=4)
    return ok


def _diffed_list_arrays(srcs, images, counts_fn, bidx, calib, kappa):
    """list_cache("exact"): every source read now (the reference's semantics, celeste.py:203-219); the entry kept per list
    only remembers what the DEVICE holds, so that the rows that differ -- and only they -- are uploaded"""
    S = len(srcs)
    arrs = _gather_plain(srcs, images, counts_fn, bidx, calib, kappa)
    key = (id(srcs), tuple(map(id, images)), counts_fn, "exact")
    imgkey = (tuple(bidx), tuple(calib.tolist()), tuple(kappa.tolist()))
    ent = _LIST_CACHE.get(key)
    if ent is not None and ent.srcs is srcs and ent.typ.shape[0] == S and ent.imgkey == imgkey:
        _LIST_CACHE.move_to_end(key)
        t, r, c, sh = arrs
        # NaN != NaN: a NaN row is uploaded again every call, which is harmless
        diff = (t != ent.typ) | np.any(r != ent.radec, axis=1) | np.any(c != ent.counts, axis=1) | np.any(sh != ent.shape, axis=1)
        rows = np.nonzero(diff)[0]
        if rows.size <= max(S // 8, 16):
            if rows.size:
                ent.typ[rows], ent.radec[rows], ent.counts[rows], ent.shape[rows] = t[rows], r[rows], c[rows], sh[rows]
                ent.version += 1
                ent.log.append((ent.version, rows))
                del ent.log[:-16]
            return ent.typ, ent.radec, ent.counts, ent.shape
    old = _LIST_CACHE.pop(key, None)
    if old is not None:
        _ENTRY_OF.pop(id(old.typ), None)
    ent = _ListEntry()
    ent.srcs, ent.objs, ent.stamps, ent.clock, ent.imgkey = srcs, None, None, None, imgkey
    ent.typ, ent.radec, ent.counts, ent.shape = arrs
    ent.version, ent.log, ent.audit, ent.index = 0, [], 0, None
    _LIST_CACHE[key] = ent
    _ENTRY_OF[id(ent.typ)] = ent
    while len(_LIST_CACHE) > _LIST_CACHE_MAX:
        _, gone = _LIST_CACHE.popitem(last=False)
        _ENTRY_OF.pop(id(gone.typ), None)
    return arrs


def _device_sources(iset, arrs):
    """the SourceSet of `iset` holding these arrays.  Arrays that came from the list cache go up row by changed row -- or
    not at all when the device copy is current."""
    typ, radec, counts, shape = arrs
    ent = _ENTRY_OF.get(id(typ))
    if ent is None or ent.typ is not typ:
        return iset._sources(typ, radec, counts, shape)
    state = getattr(iset, "_list_state", None)
    sset = iset._srcs
    if state is not None and state[0] is ent and sset is not None and sset.S == typ.shape[0]:
        rows = ent.rows_since(state[1])
        if rows is not None and rows.size <= 256:
            if rows.size:
                sset.set_rows(rows, typ[rows], radec[rows], counts[rows], shape[rows])
            iset._list_state = (ent, ent.version)
            return sset
    sset = iset._sources(typ, radec, counts, shape)
    iset._list_state = (ent, ent.version)
    return sset


def _one_stamp(image, typ, u, shape, xlim=None, ylim=None, scale=1.0):
    """(patch or None, (y0,y1), (x0,x1)) for one source on one image."""
    iset = _image_set((image,))
    srcs = iset._sources(np.array([typ], dtype=np.int32), np.asarray(u, dtype=np.float64)[None, :],
                         np.array([[scale]]), np.asarray(shape, dtype=np.float64)[None, :])
    boxes_in = None
    if xlim is not None and ylim is not None:
        boxes_in = np.array([[int(ylim[0]), int(ylim[1]), int(xlim[0]), int(xlim[1])]], dtype=np.int32)
    patches, boxes = iset.stamps(srcs, 0, scaled=(scale != 1.0), boxes_in=boxes_in)
    y0, y1, x0, x1 = (int(v) for v in boxes[0])
    return patches[0], (y0, y1), (x0, x1)


# ---- celeste.py:114-176 -----------------------------------------------------------------------
def gen_point_source_psf_image(u, image, xlim=None, ylim=None, check_overlap=True, return_patch=True,
                               psf_grid=None, pixel_grid=None):
    """generates a PSF image (assigns density values to pixels)  -- celeste.py:114-176"""
    zeros4 = (0.0, 0.0, 0.0, 0.0)
    if pixel_grid is not None and xlim is not None and ylim is not None:
        # caller-supplied N x 2 points (celeste.py:145-152): generic evaluator
        v_s = image.equa2pixel(u)
        ctx = _field.default_context(_DEVICE)
        vals = ctx.gmm_like_2d(pixel_grid, image.weights, image.means + v_s, image.covars)
        (miny_b, maxy_b), (minx_b, maxx_b) = ylim, xlim
        patch = vals.reshape((int(maxy_b - miny_b), int(maxx_b - minx_b)), order='C')
    else:
        patch, (miny_b, maxy_b), (minx_b, maxx_b) = _one_stamp(image, 0, u, zeros4, xlim, ylim)
        if patch is None and xlim is None and ylim is None and not check_overlap:
            # overlap test disabled: redo the reference's box on the host (celeste.py:137-140)
            v_s = image.equa2pixel(u)
            bound = image.R
            minx_b, maxx_b = max(0, int(v_s[0] - bound)), min(int(v_s[0] + bound + 1), image.nelec.shape[1])
            miny_b, maxy_b = max(0, int(v_s[1] - bound)), min(int(v_s[1] + bound + 1), image.nelec.shape[0])
            if maxx_b > minx_b and maxy_b > miny_b:
                patch, _, _ = _one_stamp(image, 0, u, zeros4, (minx_b, maxx_b), (miny_b, maxy_b))
        if patch is None:
            return None, None, None
        if xlim is not None and ylim is not None:
            (miny_b, maxy_b), (minx_b, maxx_b) = ylim, xlim
    if return_patch:
        return patch, (miny_b, maxy_b), (minx_b, maxx_b)
    if psf_grid is None:
        psf_grid = np.zeros(image.nelec.shape, dtype=float)
    psf_grid[int(miny_b):int(maxy_b), int(minx_b):int(maxx_b)] = patch
    return psf_grid, (0, psf_grid.shape[0]), (0, psf_grid.shape[1])


# ---- celeste.py:99-111 ------------------------------------------------------------------------
def gen_galaxy_psf_image(src, image, return_patch=True, check_overlap=True):
    """unit-flux galaxy stamp for a SrcParams galaxy  -- celeste.py:99-111"""
    assert src.a == 1, "generating glaxay psf image for non galaxy."
    from . import celeste_galaxy_conditionals as gal_funs
    th = np.array([src.theta, src.sigma, src.phi, src.rho])
    return gal_funs.gen_galaxy_psf_image(th, src.u, image, check_overlap=check_overlap,
                                         unconstrained=False, return_patch=return_patch)


# ---- celeste.py:26-62 -------------------------------------------------------------------------
def gen_src_image(src, image, return_patch=True):
    """expected photon image of a single source: unit stamp x expected photons  -- celeste.py:26-62"""
    if src.a == 1:
        f_s, _, _ = gen_galaxy_psf_image(src, image, return_patch=return_patch)
    else:
        f_s, _, _ = gen_point_source_psf_image(src.u, image, return_patch=return_patch)
    return f_s * expected_photons(src, image)    # TypeError on None, like the reference (Q1)


def gen_src_psf_image(src, image):
    if src.a == 0:
        return gen_point_source_psf_image(src.u, image)
    elif src.a == 1:
        return gen_galaxy_psf_image(src, image)
    raise NotImplementedError("not implemented!")


def gen_src_image_jac(src, image, xlim=None, ylim=None):
    """gen_src_image and its per-pixel derivatives with respect to the source's own parameters, for one star or galaxy
    -> (planes, ylim, xlim).  planes[0] is the expected photon image on the source's box (or on the limits given), planes[1],
    planes[2] its derivatives with respect to src.u (ra, dec, per degree), and for a galaxy planes[3 .. 6] those with respect to
    theta, sigma [arcsec], phi [degrees] and rho; the integer box is held fixed (ImageSet.stamp_jacobians).  (None, None, None)
    where the source has no stamp.  No counterpart in the reference, whose galaxy_source_like_grad differences whole
    likelihoods."""
    if src.a == 1:
        typ, shape = 1, [src.theta, src.sigma, src.phi, src.rho]
    elif src.a == 0:
        typ, shape = 0, (0.0, 0.0, 0.0, 0.0)
    else:
        raise NotImplementedError("gen_src_image_jac: a star (a = 0) or a galaxy (a = 1)")
    iset = _image_set((image,))
    srcs = iset._sources(np.array([typ], dtype=np.int32), np.asarray(src.u, dtype=np.float64)[None, :],
                         np.array([[expected_photons(src, image)]]), np.asarray(shape, dtype=np.float64)[None, :])
    boxes_in = None
    if xlim is not None and ylim is not None:
        boxes_in = np.array([[int(ylim[0]), int(ylim[1]), int(xlim[0]), int(xlim[1])]], dtype=np.int32)
    planes, boxes = iset.stamp_jacobians(srcs, 0, scaled=True, boxes_in=boxes_in)
    if planes[0] is None:
        return None, None, None
    y0, y1, x0, x1 = (int(v) for v in boxes[0])
    return planes[0], (y0, y1), (x0, x1)


# ---- celeste.py:193-199 -----------------------------------------------------------------------
def gen_psf_src_image_bound(src, img):
    """radius about the source's pixel position that holds 1 - epsilon of its photons in this image: the band's PSF radius
    img.R for a star, the 42-component radius of gen_galaxy_psf_image_bound for a galaxy  -- celeste.py:193-199 (the caller
    pattern of experiments/fields/process_field.py:107-117 forms floor/ceil boxes from it)"""
    if src.a == 0:
        return img.R
    from . import celeste_galaxy_conditionals as gal_funs
    return gal_funs.gen_galaxy_psf_image_bound(src, img)


# ---- celeste.py:72-96 -------------------------------------------------------------------------
def gen_point_source_psf_image_with_fluxes(src_params, fits_image, return_patch=True, psf_grid=None):
    src_img, ylim, xlim = gen_point_source_psf_image(src_params.u, fits_image, return_patch=True,
                                                     psf_grid=psf_grid)
    flux = src_params.flux_dict[fits_image.band]
    src_img = src_img * ((flux / fits_image.calib) * fits_image.kappa)
    return src_img, ylim, xlim


def gen_src_image_with_fluxes(src, img):
    """counts-scaled patch, star or galaxy, flux_dict convention  -- celeste.py:84-96"""
    scale = (src.flux_dict[img.band] / img.calib) * img.kappa
    if src.a == 1:
        patch, (y0, y1), (x0, x1) = _one_stamp(img, 1, src.u, [src.theta, src.sigma, src.phi, src.rho],
                                               scale=scale)
        return patch, (float(y0), float(y1)), (float(x0), float(x1))
    return _one_stamp(img, 0, src.u, (0.0, 0.0, 0.0, 0.0), scale=scale)


# ---- celeste.py:203-219 -----------------------------------------------------------------------
def gen_model_image(srcs, image):
    """pixel-wise mean counts: epsilon + sum of source images  -- celeste.py:203-219"""
    iset = _image_set((image,))
    typ, radec, counts, shape = _source_arrays(srcs, (image,))
    iset.render(_device_sources(iset, (typ, radec, counts, shape)), loglik=False)
    return iset.model_images()[0]


# ---- celeste.py:222-234 -----------------------------------------------------------------------
def gen_src_prob_layers(srcs, img):
    """(S+1, H, W) responsibilities: epsilon/lambda, F_s/lambda  -- celeste.py:222-234"""
    iset = _image_set((img,))
    typ, radec, counts, shape = _source_arrays(srcs, (img,))
    sset = iset._sources(typ, radec, counts, shape)
    iset.render(sset, loglik=False)
    lam = iset.model_images()[0]
    patches, boxes = iset.stamps(sset, 0, scaled=True)
    probs = np.zeros((len(srcs) + 1,) + lam.shape)
    probs[0] = img.epsilon / lam
    for s, p in enumerate(patches):
        if p is not None:
            y0, y1, x0, x1 = boxes[s]
            probs[s + 1, y0:y1, x0:x1] = p / lam[y0:y1, x0:x1]
    return probs


def estep_statistics(srcs, imgs):
    """What celeste_em reduces gen_src_prob_layers to (celeste_em.py:38-91), without building the
    (S+1, H, W) layers -- usable at 10 000 sources x 2048^2 where the layers would need 335 GB/band:
        X_tildes[s, n] = sum(all_src_probs[n][s+1] * imgs[n].nelec)          (celeste_em.py:85)
        sum_fs[s, n]   = min(1, sum(unit stamp of source s in image n))      (celeste_em.py:89)
                         -- over the UNMASKED pixels of its box in an image built with mask_invvar=True, as X_tildes and noise
        noise[n]       = sum(imgs[n].nelec * src_probs[0])                   (celeste_em.py:62, x size)
    -> (X_tildes (S, N), sum_fs (S, N), noise (N,))"""
    imgs = list(imgs)
    S = len(srcs)
    X, F, Z = np.zeros((S, len(imgs))), np.zeros((S, len(imgs))), np.zeros(len(imgs))
    i = 0
    while i < len(imgs):
        j = i + 1
        while j < len(imgs) and j - i < 16 and imgs[j].nelec.shape == imgs[i].nelec.shape:
            j += 1
        group = tuple(imgs[i:j])
        iset = _image_set(group)
        typ, radec, counts, shape = _source_arrays(srcs, group)
        xt, ms, nz = iset.estep_stats(iset._sources(typ, radec, counts, shape))
        X[:, i:j], F[:, i:j], Z[i:j] = xt, np.minimum(1.0, ms), nz
        i = j
    return X, F, Z


# ---- celeste.py:237-252 -----------------------------------------------------------------------
def celeste_likelihood(srcs, image):
    """Poisson log-likelihood sum(nelec*log(lambda) - lambda)  -- celeste.py:237-240"""
    iset = _image_set((image,))
    typ, radec, counts, shape = _source_arrays(srcs, (image,))
    total, _ = iset.render(_device_sources(iset, (typ, radec, counts, shape)), loglik=True)
    return total


def celeste_likelihood_multi_image(srcs, images):
    """sum of celeste_likelihood over images  -- celeste.py:243-252"""
    ll = 0
    images = list(images)
    i = 0
    while i < len(images):
        # consecutive images of one shape share a device image set (<= 16 per set)
        j = i + 1
        while j < len(images) and j - i < 16 and images[j].nelec.shape == images[i].nelec.shape:
            j += 1
        group = tuple(images[i:j])
        iset = _image_set(group)
        typ, radec, counts, shape = _source_arrays(srcs, group)
        total, _ = iset.render(_device_sources(iset, (typ, radec, counts, shape)), loglik=True)
        ll += total
        i = j
    return ll


def _counts_per_flux(srcs, images):
    """(S, N) d counts / d flux of expected_photons' conventions: kappa / calib (nmgy2counts: stars and galaxies), kappa
    (a is None, fluxes given); NaN for a star given by temperature (its counts do not come from its fluxes)"""
    from .celeste_src import SrcCatalog
    calib = np.array([im.calib for im in images], dtype=np.float64)
    kappa = np.array([im.kappa for im in images], dtype=np.float64)
    if isinstance(srcs, SrcCatalog):
        a = np.asarray(srcs.a)
        return np.where((a >= 0)[:, None], (kappa / calib)[None, :], kappa[None, :])
    out = np.empty((len(srcs), len(images)))
    for s, src in enumerate(srcs):
        if src.a == 0 and src.t:
            out[s] = np.nan
        elif src.a is None:
            out[s] = kappa
        else:
            out[s] = kappa / calib
    return out


def celeste_likelihood_multi_image_grad(srcs, images):
    """celeste_likelihood_multi_image and its gradient with every source's box held fixed (cel_loglik_grad), images grouped
    as celeste_likelihood_multi_image groups them.  -> (ll, {"u": (S, 2) per degree, "counts": (S, N) per image,
    "fluxes": (S, 5) through expected_photons' convention, "shape": (S, 4) theta, sigma, phi, rho})"""
    images = list(images)
    S = len(srcs)
    ll = 0
    g_u, g_shape = np.zeros((S, 2)), np.zeros((S, 4))
    g_counts = np.zeros((S, len(images)))
    i = 0
    while i < len(images):
        j = i + 1
        while j < len(images) and j - i < 16 and images[j].nelec.shape == images[i].nelec.shape:
            j += 1
        group = tuple(images[i:j])
        iset = _image_set(group)
        typ, radec, counts, shape = _source_arrays(srcs, group)
        total, gr, gc, gs = iset.loglik_grad(_device_sources(iset, (typ, radec, counts, shape)))
        ll += total
        g_u += gr
        g_shape += gs
        g_counts[:, i:j] = gc
        i = j
    g_flux = np.zeros((S, len(BANDS)))
    per = _counts_per_flux(srcs, images)
    for n, im in enumerate(images):
        g_flux[:, list(BANDS).index(im.band)] += g_counts[:, n] * per[:, n]
    return ll, {"u": g_u, "counts": g_counts, "fluxes": g_flux, "shape": g_shape}
