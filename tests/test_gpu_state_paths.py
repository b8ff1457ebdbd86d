"""Stored state on every path, not only verdicts: the sequences the knob and path variants of
test_gpu_parity.py run, with the exported history compared against the semantic oracle's canonical
form after every batch (tests/export_helpers.Pair).  A merge that stores a wrong version or
misplaces a boundary on one of those paths fails here at the batch that stored it, whether or not
a later read of the same short sequence happens to land on it."""
import numpy as np
import pytest

from foundationdb_amd import workloads as W
from tests.export_helpers import Pair
from tests.helpers import (PIPELINE_KNOBS, SORT_BUCKETS, pipeline_variant_batches,
                           sequential_fallback_batches, sort_bucket_batches)

pytestmark = pytest.mark.gpu


def _id(knobs):
    return "-".join(f"{k[6:]}={v}" for k, v in knobs.items())


def make_pair(monkeypatch, knobs, *args, **kw):
    """The knobs stand for the whole test: most are read when the set is created, FDBCS_EDGE_CAP when
    the first batch sizes the workspace."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    return Pair(*args, **kw)


def run_checked(pair, seq):
    for i, (pb, now, new_oldest) in enumerate(seq):
        pair.detect(pb, now, new_oldest)  # verdicts and reports equal the oracle's
        pair.check(what=i)


@pytest.mark.parametrize("knobs", PIPELINE_KNOBS + [{"FDBCS_RESOLVE_PREPASS": "0"}, {"FDBCS_DIR_BITS": "4"},
                                                    {"FDBCS_DIR_BITS": "20"}], ids=_id)
def test_pipeline_variants_store_the_oracle_state(engine, oracle_built, monkeypatch, knobs):
    """The 20 batches of test_pipeline_variants_match_oracle (keys up to 3, 24 and 40 bytes,
    a compaction every few batches) under every knob set it lists, the resolution without its
    pre-pass, and the smallest and a large radix directory."""
    pair = make_pair(monkeypatch, knobs, engine, oracle_built, gc_interval=0, delta_limit=400)
    run_checked(pair, pipeline_variant_batches())
    assert pair.cs.history_size() > 0


@pytest.mark.parametrize("bucket,cold", SORT_BUCKETS)
def test_sort_bucket_sizes_store_the_oracle_state(engine, oracle_built, monkeypatch, bucket, cold):
    pair = make_pair(monkeypatch, {"FDBCS_SORT_BUCKET": bucket, "FDBCS_SORT_COLD": cold}, engine, oracle_built)
    run_checked(pair, sort_bucket_batches())
    if bucket in ("3000", "600"):
        assert pair.cs.stats()["sort_big_buckets"] > 0  # the workgroup path ran


def test_sequential_fallback_stores_the_oracle_state(engine, oracle_built, monkeypatch):
    pair = make_pair(monkeypatch, {"FDBCS_EDGE_CAP": "8"}, engine, oracle_built)
    run_checked(pair, sequential_fallback_batches())
    assert pair.cs.stats()["intra_fallbacks"] > 0  # the fallback was taken


@pytest.mark.parametrize("prepass", ["1", "0"])
def test_c3_zipf_stores_the_oracle_state(engine, oracle_built, monkeypatch, prepass):
    """Zipf hot keys (C3's shape): 1500 transactions of 5 reads and 2 writes, hundreds of candidate
    writers per hot key, 4 batches, with the resolution's pre-pass and without it."""
    p = W.C2Params(txns=1500)
    z = W.ZipfGenerator(1_000_000, 0.99)
    rng = np.random.default_rng(3)
    pair = make_pair(monkeypatch, {"FDBCS_RESOLVE_PREPASS": prepass}, engine, oracle_built)
    now = 1_000_000
    seen = set()
    for i in range(4):
        now += 1000
        seen |= set(pair.detect(W.c3_batch(p, rng, now, z), now, now - 100_000).tolist())
        pair.check(what=i)
    assert {0, 2} <= seen  # conflicts and commits


@pytest.mark.parametrize("submit_thread", ["0", "1"])
def test_async_batches_store_the_oracle_state(engine, oracle_built, monkeypatch, submit_thread):
    """Eight batches submitted with detect_async, four in flight; the state is compared once, after
    the last wait (an export refuses while a batch is unwaited)."""
    rng = np.random.default_rng(4)
    pair = make_pair(monkeypatch, {"FDBCS_SUBMIT_THREAD": submit_thread}, engine, oracle_built, gc_interval=0,
                     delta_limit=300)
    now = 10
    inflight = []

    def wait_first():
        b, want = inflight.pop(0)
        assert (b.wait() == want).all()
        b.close()

    for _ in range(8):
        pb = W.random_small_batch(rng, 200, alphabet=4, max_len=4, now=now, staleness=10)
        b = engine.ConflictBatch(pair.cs)
        b.add_packed(pb)
        b.upload()
        b.detect_async(now, now - 5)
        inflight.append((b, pair.o.detect(pb, now, now - 5)[0]))
        if len(inflight) == 4:
            wait_first()
        now += 2
    while inflight:
        wait_first()
    pair.check(what="after the last wait")
