"""The audit of tests/thresholds.py; needs no GPU.

  1. Every constant the table restates equals the `constexpr int NAME = value` of the kernel source: a retune breaks the
     audit instead of silently moving a boundary.
  2. Every case reaches the regimes it claims — computed from the case's inputs and the oracle's outputs, never from the
     library — whether tests/test_gpu_thresholds.py runs it or an older GPU test does.
  3. Every regime of every row has a case, every row has a case below, at and above its constant, and every new case is
     the only one in some regime: removing any of them fails here, with the uncovered regime by name.
The report (-s, or the failure text) lists, row by row, the cases below, at and above the threshold."""
import os

import pytest

import thresholds as T


def test_restated_constants_equal_the_kernel_sources():
    parsed = {}
    for row in T.ROWS:
        path = os.path.join(T.CSRC, row["file"])
        src = parsed.setdefault(row["file"], T.parse_constants(path))
        for name, value in row["constants"].items():
            assert name in src, "%s: no `constexpr int %s` in %s" % (row["id"], name, row["file"])
            assert src[name] == value, "%s: the table says %s = %d, %s says %d" % (row["id"], name, value, row["file"], src[name])


def test_the_table_is_well_formed():
    for row in T.ROWS:
        keys = [g["key"] for g in row["regimes"]]
        assert len(set(keys)) == len(keys), row["id"]
        assert all(g["side"] in ("below", "at", "above") for g in row["regimes"]), row["id"]
    for c in T.CASES:
        for row, keys in c["claims"].items():
            assert row in T.ROW and set(keys) <= {g["key"] for g in T.ROW[row]["regimes"]}, (c["id"], row, keys)


@pytest.mark.parametrize("case", T.CASES, ids=[c["id"] for c in T.CASES])
def test_case_reaches_the_regimes_it_claims(case):
    reached = T.classify(case["id"])
    for row, keys in case["claims"].items():
        assert set(keys) <= reached.get(row, set()), "%s: claims %s of %s, reaches %s" % (case["id"], keys, row, sorted(reached.get(row, ())))


def report():
    cov = T.coverage()
    lines = []
    for row in T.ROWS:
        lines.append("%s  [%s; %s]  %s" % (row["id"], row["kernel"], ", ".join("%s = %d" % kv for kv in row["constants"].items()),
                                            row["quantity"]))
        for side in ("below", "at", "above"):
            for g in row["regimes"]:
                if g["side"] == side:
                    lines.append("    %-5s  %-42s %s" % (side, g["key"], ", ".join(cov[row["id"]][g["key"]]) or "-- NO CASE --"))
    return "\n".join(lines)


def test_every_regime_has_a_case_below_at_and_above():
    text = report()
    print("\n" + text)
    missing = T.uncovered()
    assert not missing, "uncovered: %s\n%s" % ("; ".join("%s: %s" % m for m in missing), text)


def test_every_new_case_is_needed():
    """Without any one of the new cases some regime is left without a case, and `uncovered` names it."""
    for c in T.new_cases():
        rest = [x for x in T.CASES if x is not c]
        missing = T.uncovered(rest)
        assert missing, "%s could be removed without the audit noticing" % c["id"]
        assert all(row in c["claims"] for row, _ in missing), (c["id"], missing)


def test_existing_cases_are_the_inputs_of_a_test_that_exists():
    """An `origin` names a GPU test and, where it is parametrised, one of its parameter sets. The test must still have that
    parameter set, the case must restate its values, and the test's body must still seed its generator (and, for the ROI
    case, shape its map) the way the builder in thresholds.py does — the builders call the tests' own helpers
    (`adl_case`, `random_rois`) for everything else."""
    import ast
    for c in T.CASES:
        if c["origin"] == "new":
            continue
        path, name = c["origin"].split("::")
        name, _, pid = name.partition("[")
        with open(os.path.join(T.ROOT, path)) as fh:
            source = fh.read()
        fn = {n.name: n for n in ast.parse(source).body if isinstance(n, ast.FunctionDef)}.get(name)
        assert fn is not None, c["origin"]
        body = ast.get_source_segment(source, fn)
        if pid:
            sets = {}
            for dec in fn.decorator_list:
                if isinstance(dec, ast.Call) and ast.unparse(dec.func) == "pytest.mark.parametrize":
                    names = [a.strip() for a in ast.literal_eval(dec.args[0]).split(",")]
                    for values in ast.literal_eval(dec.args[1]):
                        sets["-".join(str(v) for v in values)] = dict(zip(names, values))
            assert pid.rstrip("]") in sets, "%s: %s has no such parameter set (it has %s)" % (c["id"], name, sorted(sets))
            for k, v in sets[pid.rstrip("]")].items():
                assert c[k] == v, "%s: %s = %r in the table, %r in %s" % (c["id"], k, c[k], v, c["origin"])
            assert "default_rng(%d)" % c["seed"] in body, c["origin"]
        if c["op"] == "roi_bwd":
            d = T.build(c["id"])
            assert "default_rng(14)" in body and "B, H, W, C = %d, %d, %d, %d" % d["data"].shape in body
            assert "random_rois(rng, %d, B, C, W * 8, H * 8)" % c["R"] in body and "3, 3, 0.125" in body
