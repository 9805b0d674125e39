"""CPU: which branches of the V11 SIFT the seeded inputs of tests/sift_cases.py take, counted by
the census of the restatement (tests/sift_ref.py).  tests/test_gpu_sift_shapes.py compares the
kernels with the restatement on exactly these inputs, so a branch counted here is a branch held
there.  MEASURED is what the committed recipes give, summed over all cases (the table per case is
in DESIGN.md K7 and is printed by test_every_branch_is_reached); the floor of each counter is half
of it, at least 1."""
import numpy as np

import sift_cases as cs
import sift_ref as sr
import sift_scenes as sc

MEASURED = {
    # detect
    "start": 1795, "det0": 2, "offset_above_2^20": 1, "conv_solve_1": 1307, "conv_solve_2": 101, "conv_solve_3": 21,
    "conv_solve_4": 2, "conv_solve_5": 2, "no_conv_after_5": 226, "move": 1347, "move_level": 479, "leave_level": 129,
    "leave_rowcol": 4, "contrast": 4, "d2": 5, "edge": 51, "edge_both_sides_equal": 1, "scale_ol>=0": 617,
    "scale_ol<0": 756, "kept_level_1": 677, "kept_level_2": 545, "kept_level_3": 151, "records": 1373,
    # orient
    "orient_records": 8979, "orient_out_of_contract": 28, "peaks_0": 784, "peaks_1": 6243, "peaks_2": 1567,
    "peaks_3": 303, "peaks_4": 51, "peaks_above_4": 3, "peak_in_bin_0": 1836, "peak_in_bin_35": 836, "q_wrap": 25,
    "hist_term_at_bound": 26851, "oriented": 10502,
    # describe
    "describe_rows": 18738, "describe_out_of_contract": 28, "zero_norm": 187, "entry_clamped_255": 724,
}


def columns():
    """(name, census) per case, in the order of the table of DESIGN.md K7."""
    cols = [("batch %d" % v, b["census"]) for v, b in enumerate(cs.batch())]
    cols += [("150x203 " + k, r["census"]) for k, r in cs.small()["runs"].items()]
    cols += [("planted " + k, r["census"]) for k, r in cs.planted().items()]
    cols += [("planted iso", cs.planted(("iso",))["iso"]["census"])]
    cols += [("edge 1: planted " + k, r["census"]) for k, r in cs.planted_tie().items()]
    cols += [("random", cs.random_case()["census"]), ("steep", cs.steep_case()["census"]),
             ("contract", cs.contract_case()["census"])]
    return cols


def test_every_branch_is_reached():
    cols = columns()
    keys = []
    for _, c in cols:
        keys += [k for k in c if k not in keys]
    total = {k: sum(c.get(k, 0) for _, c in cols) for k in keys}
    print("| counter | " + " | ".join(n for n, _ in cols) + " | all |")
    print("|---|" + "---|" * (len(cols) + 1))
    for k in keys:
        print("| %s | " % k + " | ".join(str(c[k]) if k in c else "" for _, c in cols) + " | %d |" % total[k])
    print("MEASURED =", total)
    assert set(total) == set(MEASURED), sorted(set(total) ^ set(MEASURED))
    low = {k: (total[k], MEASURED[k]) for k in MEASURED if total[k] < max(1, MEASURED[k] // 2)}
    assert not low, low


def test_batch_counts_and_the_emit_carry():
    """The counts the GPU batch test relies on: more than one 256-record chunk in views 0 and 2
    (the carry of sift_orient_emit_kernel), none at all in view 1."""
    b = cs.batch()
    assert [v["rec"].shape[0] for v in b] == [323, 0, 321]
    assert [v["orec"].shape[0] for v in b] == [438, 0, 478]
    assert np.bincount(b[0]["rec"][:, 0], minlength=4).tolist() == [277, 44, 2, 0]
    # a record beyond the first chunk with a peak, and records before it with more than one: the
    # carry is not 256 and not the records' own index
    for v in (0, 2):
        assert b[v]["rec"].shape[0] > 256 and b[v]["orec"].shape[0] > b[v]["rec"].shape[0]


def test_parameter_runs_differ():
    r = cs.small()["runs"]
    n = {k: v["rec"].shape[0] for k, v in r.items()}
    print(n)
    assert n["default"] == 140 and n["edge3"] == 110 and r["edge3"]["census"]["edge"] == 31
    assert n["contrast.08"] < n["default"] and r["contrast.08"]["census"]["contrast"] >= 1
    assert n["border1"] > n["default"] > n["border40"] >= 1


def test_planted_branches_exactly_once():
    p = cs.planted()
    assert p["det0"]["census"]["det0"] == 1 and p["det0"]["census"]["offset_above_2^20"] == 0
    assert p["big"]["census"]["offset_above_2^20"] == 1 and p["big"]["census"]["det0"] == 0
    # the two negative diagonals of a stencil are minima of their own: two ordinary records
    assert p["det0"]["rec"].shape[0] == 2 and p["big"]["rec"].shape[0] == 2
    m = p["move"]["census"]
    assert m["leave_rowcol"] == 1 and m["leave_level"] == 0 and m["move"] >= 1 and m["move_level"] == 0
    assert p["zero"]["rec"].shape[0] == 0 and p["zero"]["census"] == {"start": 0}
    # the isotropic stencil: a record at edge ratio 10, rejected at 1 where both sides are equal
    assert cs.planted(("iso",))["iso"]["rec"].shape[0] == 1
    t = cs.planted_tie()["iso"]
    assert t["rec"].shape[0] == 0 and t["census"]["edge_both_sides_equal"] == 1 and t["census"]["edge"] == 1


def test_census_changes_nothing():
    tb = cs.tables()
    octs = cs.small()["octs"]
    rec = sr.detect(octs, tb)
    assert np.array_equal(rec, cs.small()["runs"]["default"]["rec"])
    some = sc.random_records(octs, 300, 9)
    cen = {}
    orec = sr.orient(octs, some, tb)
    assert np.array_equal(orec, sr.orient(octs, some, tb, census=cen))
    assert np.array_equal(sr.describe(octs, orec, tb), sr.describe(octs, orec, tb, census=cen))
    assert cen["orient_records"] == 300 and cen["describe_rows"] == orec.shape[0]


def test_records_outside_the_contract():
    """They give no oriented record and a zero descriptor row, and their valid neighbours what they
    give without them."""
    c = cs.contract_case()
    assert sr.in_contract(np.stack([cs.mk(*r) for r in cs.OUTSIDE]), 4).sum() == 0
    assert sr.in_contract(np.stack([cs.mk(*r) for r in cs.INSIDE]), 4).all()   # the bounds themselves are inside
    for v in c["views"]:
        assert v["bad"].sum() == len(cs.OUTSIDE) and np.array_equal(v["orec"], v["good_orec"])
        assert not v["qdesc"][v["bad"]].any() and v["qdesc"][~v["bad"]].any(1).sum() >= 20
        assert np.array_equal(v["qdesc"][~v["bad"]], sr.describe(c["octs"], v["qrec"][~v["bad"]], cs.tables()))
