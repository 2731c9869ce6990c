"""A whole step of the receiver bank, pinned: every kg_rxbank_step_info field (table_bytes included), the audio, frame, spectrum and
extension maps and the SHA-256 of each bank buffer's written extent, over the eighteen steps of tests/rxbank_fingerprint.py -- two
overlapped receivers and a ring wrap, all six mode families, the audio spectrum with a channel null, the FFT extension on two receivers,
both blankers, a leave, a join and a `SET mod=`.  The fixture was recorded from the library as it was before the step was split into
plan / enqueue / commit (tools/make_rxbank_fingerprint_golden.py); equality, no tolerance: the same kernels get the same arguments."""
import os

import numpy as np
import pytest

from . import rxbank_fingerprint as fp

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rxbank_fingerprint.npz")


def test_whole_step_fingerprint():
    want = np.load(GOLDEN)
    got = fp.run()
    fp.check_preconditions(got)
    buffers = [str(b) for b in want["buffers"]]
    assert set(fp.MUST_HOLD) <= set(buffers)
    for j, f in enumerate(fp.INFO_FIELDS):
        assert got["info"][:, j].tolist() == want["info"][:, j].tolist(), f
    for k in ("audio_map", "frame_n", "frame_map", "spec_n", "spec_map", "fftext_n", "fftext_map"):
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (k, "first difference at [step, ...]", bad[0].tolist())
    for b in buffers:
        bad = np.flatnonzero(got["digest_" + b] != want["digest_" + b])
        assert bad.size == 0, (b, "digest differs on steps", bad.tolist())
