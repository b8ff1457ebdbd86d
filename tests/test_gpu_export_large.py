"""The export's key-byte offsets past 2^32: the scan carries 32-bit components, and only an export of
more than 4 GiB of key bytes shows whether the 64-bit offsets rebuilt from them are exact."""
import numpy as np
import pytest

from tests.export_helpers import NO_FLOOR

pytestmark = pytest.mark.gpu


def test_key_bytes_past_4gib(engine):
    L, n = 4101, 1_060_000  # 4.35e9 bytes of keys: tails of 511 words, offsets of every alignment
    assert n * L > (1 << 32) + (1 << 24)
    i = np.arange(n, dtype=np.int64)
    keys = np.add.outer((i % 251).astype(np.uint8) * np.uint8(7), np.arange(L, dtype=np.uint8))
    keys[:, :8] = i.astype(">u8").view(np.uint8).reshape(n, 8)  # strictly ascending
    kb = keys.reshape(-1)
    ko = np.arange(n + 1, dtype=np.int64) * L
    vers = (i % 2) + 5
    cs = engine.ConflictSet()
    cs.load_history(kb, ko, vers, 0)
    kb2, ko2, vv2, hdr = cs.dump_history(floor=NO_FLOOR)
    cs.close()
    assert hdr == 0
    assert np.array_equal(ko2, ko)
    assert np.array_equal(vv2, vers)
    assert np.array_equal(kb2, kb)
