"""The device add's directed plan (tests/device_add_plan.py) held to the semantic oracle, on the CPU:
its verdicts are the ones it was built for, and every defined mutation of every class's key, as a
range's begin and as its end, changes a verdict (reads) or the stored state (writes).  Without this
the GPU parity test could pass with a normalization that mangles some class of keys."""
import numpy as np
import pytest

from foundationdb_amd.packing import InvertedRange, KeyRange
from tests import device_add_plan as P


def fresh(oracle):
    cs = oracle.OracleConflictSet()
    cs.load_history(*P.history())
    return cs


@pytest.fixture(scope="module")
def plan_run(oracle_built):
    cs = fresh(oracle_built)
    out = []
    for pb, now, oldest in P.sequence():
        v, conf = cs.detect(pb, now, oldest)
        out.append((v, conf, cs.dump_history()))
    return out


def test_classes_cover_the_lengths():
    assert sorted({c.n for c in P.CLASSES}) == sorted(set(P.LENGTHS))
    ties = [c for c in P.CLASSES if c.name.startswith("tie")]
    assert [c.ka[-1] for c in ties] == [0, 0] and [len(c.ka) for c in ties] == [17, 18]
    k16 = P.CLASSES[P.LENGTHS.index(16)]
    assert len(k16.ka) == 16
    for c in ties:  # the tie's neighbour below is the 16-byte key itself (or the tie before it)
        assert P.pred_of(c.ka)[:16] == c.ka[:16] and P.pred_of(c.kb)[:16] == c.kb[:16]


def test_plan_verdicts(plan_run):
    (v0, conf0, _), (v1, _, _), (v2, conf2, _) = plan_run
    np.testing.assert_array_equal(v0, P.want_read_verdicts())
    nk = len(P.write_keys())
    assert v1.tolist() == [2] * nk + [1, 2]
    assert v2.tolist() == [0, 2, 2] * nk
    assert {0, 1, 2} <= set(np.concatenate([v0, v1, v2]).tolist())
    assert any(conf0.values()) and any(conf2.values())
    assert all(conf0[t] == [0] for t in np.flatnonzero(v0 == 0))


def test_written_keys_are_stored_exactly(plan_run):
    keys, vers = plan_run[1][2]
    at = dict(zip(keys, vers.tolist()))
    for k in P.write_keys():
        assert at.get(k) == P.NOW_WRITES, k
        assert k + b"\x00" in at and at[k + b"\x00"] != P.NOW_WRITES
    assert b"\xf0too-old" not in at and at.get(b"\xf2") == P.NOW_WRITES


@pytest.mark.parametrize("how", P.MUTATIONS)
def test_every_read_mutation_changes_a_verdict(oracle_built, plan_run, how):
    base = plan_run[0][0]
    defined = 0
    for i, c in enumerate(P.CLASSES):
        for side, k in (("a", c.ka), ("b", c.kb)):
            m = P.mutate(k, how)
            if m is None:
                continue
            defined += 1
            v, _ = fresh(oracle_built).detect(P.read_batch((i, side, m)), P.NOW_READS, P.OLDEST_AFTER_READS)
            assert (v != base).any(), (c.name, side, how)
            assert (v != base)[: 4 * i].sum() == 0 and (v != base)[4 * i + 4:].sum() == 0
    # undefined only where the docstring says: no byte to drop or zero, a trailing \0 zeroed, fewer
    # than two (or two equal) bytes past 16 to rotate
    want = {"drop": 2 * len(P.CLASSES) - 2, "zero": 2 * (len(P.CLASSES) - 1 - len(P.TIES)),
            "append": 2 * len(P.CLASSES),
            "rotate": 2 * sum(1 for c in P.CLASSES if c.n >= 18 and not c.name.startswith("tie"))}
    assert defined == want[how]


@pytest.mark.parametrize("how", P.MUTATIONS)
def test_every_write_mutation_changes_the_state(oracle_built, plan_run, how):
    keys0, vers0 = plan_run[1][2]
    wk = P.write_keys()
    for j, k in enumerate(wk):
        for end in (False, True):
            m = P.mutate(k + b"\x00" if end else k, how)
            if m is None:
                continue
            ranges = [(x, x + b"\x00") for x in wk]
            ranges[j] = (k, m) if end else (m, k + b"\x00")
            try:
                KeyRange(*ranges[j])
            except InvertedRange:
                continue  # refused outright: no valid batch holds it
            cs = fresh(oracle_built)
            cs.detect(P.read_batch(), P.NOW_READS, P.OLDEST_AFTER_READS)
            cs.detect(P.write_batch(ranges), P.NOW_WRITES, P.OLDEST_AFTER_READS)
            keys, vers = cs.dump_history()
            assert keys != keys0 or vers.tolist() != vers0.tolist(), (k, end, how)
