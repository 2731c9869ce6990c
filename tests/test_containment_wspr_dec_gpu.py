"""What kg_wspr_decode may write: the records and counts of the entries it was given, and the ignore flags of the connections listed.
Non-finite samples are undefined as in the reference; whatever they give, the connections listed beside them get the records they get
alone, the caller's bytes around `out` and `ncand` stay the caller's, and nothing is left allocated."""
import ctypes as C

import numpy as np
import pytest

from flydog_sdr_gps_amd import Context, Wspr, live_allocs, wspr
from flydog_sdr_gps_amd._lib import check, ptr

from . import wspr_dec_common as W

pytestmark = pytest.mark.gpu
FILL = 0xA5


def test_non_finite_samples_stay_inside_the_connection():
    g = W.load()
    ctx = Context(0)
    q = Wspr(ctx, nconn=3)
    q.set_metric_table(g["mettab"])
    for c in range(3):
        q.init(c, 375.0)
    scene = {0: "jig_a", 2: "twelve"}
    alone = {}
    for c, name in scene.items():
        x, cands, _ = W.scene_inputs(name)
        q.load_iq(c, 0, x, [tuple(v) for v in cands.tolist()])
        alone[c] = q.decode([c], 200, 2)
        q.load_iq(c, 0, x, [tuple(v) for v in cands.tolist()])                                               # ignore cleared again
    x, cands, _ = W.scene_inputs("strong")
    bad = x.copy()
    bad[1000] = np.nan
    bad[5000] = np.inf + 0j
    bad[20000] = complex(-np.inf, np.nan)
    bad[44999] = complex(3e38, 3e38)
    bad_cands = [tuple(v) for v in cands.tolist()] + [(-20.0, 4900, 2.0, 0.1)]
    q.load_iq(1, 1, bad, bad_cands)
    q.decode([0, 1, 2], 1, 128, True)                                                                        # the workspace for three connections exists from here on
    for c, name in scene.items():
        xs, cs, _ = W.scene_inputs(name)
        q.load_iq(c, 0, xs, [tuple(v) for v in cs.tolist()])
    q.load_iq(1, 1, bad, bad_cands)
    allocs = live_allocs()
    raw = np.full(304 * (3 * 12 + 2), FILL, np.uint8)
    cnt = np.full(5, FILL | (FILL << 8) | (FILL << 16) | (FILL << 24), np.uint32).view(np.int32)
    conns = np.array([0, 1, 2], np.int32)
    check(q.lib.kg_wspr_decode(q.h, ptr(conns), 3, 200, 2, 0, C.c_void_p(raw.ctypes.data + 304), C.c_void_p(cnt.ctypes.data + 4)), "kg_wspr_decode")
    assert (raw[:304] == FILL).all() and (raw[-304:] == FILL).all() and cnt.view(np.uint32)[0] == cnt.view(np.uint32)[4] == 0xA5A5A5A5
    out = raw[304:-304].view(wspr.dec_dtype).reshape(3, 12)
    assert cnt[1:4].tolist() == [1, 2, 12]
    for e, c in ((0, 0), (2, 2)):
        assert out[e].tobytes() == alone[c][0][0].tobytes(), scene[c]
    assert live_allocs() == allocs
    # the object goes on: finite samples in the same connection decode as ever
    q.load_iq(1, 1, x, [tuple(v) for v in cands.tolist()])
    got = q.decode([1], 200, 2)[0][0][:1]
    want = np.ascontiguousarray(g["s_strong_recs"]).view(W.rec_dtype)[..., 0][0]
    assert got.tobytes() == want.tobytes()
    q.close()
    ctx.close()
