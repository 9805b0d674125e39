"""The seeded SIFT inputs shared by tests/test_sift_census_cpu.py (which branches of the
restatement they take) and tests/test_gpu_sift_shapes.py (the kernels against the restatement on
them).  Every case is computed once per process and handed out read-only."""
import functools
import importlib

import numpy as np

import sift_ref as sr
import sift_scenes as sc

BATCH = ((233, 301, 1, (3, 7)), None, (233, 301, 5, (4,)))   # None: a constant image of 200
SMALL = (150, 203, 1, (3, 7))
# detect on the 150 x 203 texture: (name, keyword arguments)
PARAMS = (("edge3", dict(edge=3.0)), ("contrast.01", dict(contrast=0.01)), ("contrast.08", dict(contrast=0.08)),
          ("border1", dict(border=1)), ("border40", dict(border=40)))
PLANTED = ("det0", "big", "move", "zero")
RANDOM_SEEDS = (101, 202)   # one per view
RANDOM_N = 4000
STEEP_N = 256


def tables():
    return importlib.import_module("3d_reconstruction_amd").sift_tables()


def _freeze(x):
    for a in (x if isinstance(x, (list, tuple)) else [x]):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def batch():
    """V = 3 at 233 x 301, O = 4: per view img, octs, rec, orec, desc and the census of each stage."""
    tb, out = tables(), []
    for spec in BATCH:
        img = np.full((233, 301), 200, np.uint8) if spec is None else sc.block_texture(*spec)
        cen = {}
        octs = sr.pyramid(img, 4, tb)
        rec = sr.detect(octs, tb, census=cen)
        orec = sr.orient(octs, rec, tb, census=cen)
        desc = sr.describe(octs, orec, tb, census=cen)
        out.append(dict(img=_freeze(img), octs=_freeze(octs), rec=_freeze(rec), orec=_freeze(orec), desc=_freeze(desc),
                        census=cen))
    return out


@functools.lru_cache(maxsize=None)
def small():
    """The 150 x 203 texture, O = 4: img, octs, and rec / census per parameter set of PARAMS."""
    tb = tables()
    img = sc.block_texture(*SMALL)
    octs = sr.pyramid(img, 4, tb)
    runs = {}
    for name, kw in (("default", {}),) + PARAMS:
        cen = {}
        runs[name] = dict(kw=kw, rec=_freeze(sr.detect(octs, tb, census=cen, **kw)), census=cen)
    return dict(img=_freeze(img), octs=_freeze(octs), runs=runs)


@functools.lru_cache(maxsize=None)
def planted(kinds=PLANTED, edge=10.0):
    """Hand-built octaves (32 x 32, O = 1), one view each: octs, rec and census per kind."""
    tb, out = tables(), {}
    for kind in kinds:
        cen = {}
        octs = [sc.planted_pyramid(kind)]
        out[kind] = dict(octs=_freeze(octs), census=cen,
                         rec=_freeze(sr.detect(octs, tb, sc.PLANT_BORDER, edge=edge, census=cen)))
    return out


def planted_tie():
    """The isotropic stencil at edge ratio 1, where both sides of the edge test are equal."""
    return planted(("iso", "det0"), 1.0)


def _with_random_q(orec, seed):
    out = orec.copy()
    q = np.random.default_rng(seed).integers(0, 1024, orec.shape[0]).astype(np.int32)
    out[:, 1] = (out[:, 1] & 0xff) | (q << 8)
    return out


def _records_case(octs, recs):
    """orient, describe of its output, and describe of the records themselves with a random q."""
    tb, views, cen = tables(), [], {}
    for v, rec in enumerate(recs):
        orec = sr.orient(octs, rec, tb, census=cen)
        qrec = _with_random_q(rec, 7 + v)
        views.append(dict(rec=_freeze(rec), orec=_freeze(orec), desc=_freeze(sr.describe(octs, orec, tb, census=cen)),
                          qrec=_freeze(qrec), qdesc=_freeze(sr.describe(octs, qrec, tb, census=cen))))
    return dict(octs=_freeze(octs), views=views, census=cen)


@functools.lru_cache(maxsize=None)
def random_case():
    """4000 random records in each of two views on the pyramid of the half-flat texture (both
    views hold the same image: the records differ)."""
    octs = sr.pyramid(sc.half_flat_texture(), 4, tables())
    return _records_case(octs, [sc.random_records(octs, RANDOM_N, s) for s in RANDOM_SEEDS])


@functools.lru_cache(maxsize=None)
def steep_case():
    """256 random records on the 150 x 203 texture's pyramid times 2^12."""
    octs = sc.steep(small()["octs"])
    return _records_case(octs, [sc.random_records(octs, STEEP_N, 303)])


def mk(o, l, x, y, s):
    r = np.zeros(8, np.int32)
    r[0], r[1] = o, l
    with np.errstate(all="ignore"):
        r[2:8] = np.array([x, y, s, 1.0, x, y], np.float32).view(np.int32)
    return r


# records outside the contract of the header: (octave, level, x, y, scale); O = 4 below
OUTSIDE = ((-1, 2, 20.0, 20.0, 2.0), (4, 2, 20.0, 20.0, 2.0), (2 ** 30, 2, 20.0, 20.0, 2.0),
           (0, 0, 20.0, 20.0, 2.0), (0, 4, 20.0, 20.0, 2.0), (0, 255, 20.0, 20.0, 2.0),
           (0, 2, 20.0, 20.0, np.nan), (0, 2, 20.0, 20.0, np.inf), (0, 2, 20.0, 20.0, 3e38), (0, 2, 20.0, 20.0, 0.0),
           (0, 2, np.nan, 20.0, 2.0), (1, 1, 20.0, -np.inf, 2.0), (0, 3, 20.0, 20.0, -2.0), (1, 2, 2.0e6, 20.0, 2.0))


# and records on the bounds of the contract, which are inside it
INSIDE = ((3, 3, 1048576.0, -1048576.0, 1048576.0), (0, 1, 30.0, 30.0, 1e-30), (0, 2, -1048576.0, 30.0, 2.0))


@functools.lru_cache(maxsize=None)
def contract_case():
    """Two views on the 150 x 203 texture's pyramid: the detector's records with the records of
    OUTSIDE planted between them (every third place in view 0, in a block and at both ends in
    view 1, followed by the records of INSIDE).  bad marks the rows of OUTSIDE."""
    tb = tables()
    octs = small()["octs"]
    valid = small()["runs"]["default"]["rec"]
    out = [np.stack([mk(*r) for r in OUTSIDE])]
    views, cen = [], {}
    for v in range(2):
        rows, bad = [], []
        if v == 0:
            for i, r in enumerate(out[0]):
                rows += [valid[2 * i], valid[2 * i + 1], r]
                bad += [False, False, True]
        else:
            rows = [out[0][0]] + list(valid[40:50]) + list(out[0][1:-1]) + list(valid[50:60]) + [out[0][-1]]
            bad = [True] + [False] * 10 + [True] * (len(OUTSIDE) - 2) + [False] * 10 + [True]
            rows += [mk(*r) for r in INSIDE]
            bad += [False] * len(INSIDE)
        rec, bad = np.stack(rows), np.array(bad)
        orec = sr.orient(octs, rec, tb, census=cen)
        qrec = _with_random_q(rec, 17 + v)
        views.append(dict(rec=_freeze(rec), bad=_freeze(bad), orec=_freeze(orec),
                          good_orec=_freeze(sr.orient(octs, rec[~bad], tb)), qrec=_freeze(qrec),
                          qdesc=_freeze(sr.describe(octs, qrec, tb, census=cen))))
    return dict(octs=octs, views=views, census=cen)
