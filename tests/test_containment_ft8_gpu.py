"""kg_ft8 takes host arrays, so what a push may write is the connection's own object on the device and the stated extents of the caller's
host arrays.  The samples are int16: nothing is non-finite, the extreme ones are -32768 (whose square wave is past full scale: the byte
chain clamps at 255) and a slot of them.  Whatever they give, they write nothing outside the object of the connection they are pushed
to -- the two connections beside it keep every byte of their state, samples' tail and waterfall included -- and nothing of the caller's
event and slot arrays beyond the counts returned.  The trees are compared with tests/guarded.py's freeze / first_difference."""
import ctypes as C

import numpy as np
import pytest

from flydog_sdr_gps_amd import Context, Ft8, ft8, live_allocs
from flydog_sdr_gps_amd._lib import check, ptr

from . import ft8_common as F
from .guarded import first_difference, freeze

pytestmark = pytest.mark.gpu
FILL = 0xA5


def tree(q, c):
    info, lf, mag = q.state(c)
    return [info.tobytes(), lf, mag, q.state(c, previous=True)[2]]


def test_extreme_samples_stay_inside_the_connection():
    ctx = Context(0)
    q = Ft8(ctx, nconn=3)
    p = F.FT4
    x, t = F.STREAMS["boundary_ft4"][1]()
    for c in range(3):
        q.init(c, p)
    q.push([0, 2], np.stack([x, x[::-1]]), np.stack([t, t]))               # a slot end and the next slot's start in both
    beside = freeze([tree(q, c) for c in (0, 2)])
    bad = x.copy()
    bad[:] = np.where(np.arange(F.NS) % 8 < 4, 32767, -32768).astype(np.int16)     # a 1500 Hz square wave, its low half past full scale
    bad[40:60] = -32768
    allocs = live_allocs()
    max_events, max_slots = 8, 1
    ev = np.zeros(max_events + 4, ft8.ev_dtype)
    sl = np.zeros(max_slots + 1, ft8.slot_dtype)
    ev.view(np.uint8)[:] = FILL
    sl.view(np.uint8)[:] = FILL
    ne, nsl = C.c_int32(0), C.c_int32(0)
    conns, ncb = np.array([1], np.int32), np.array([bad.shape[0]], np.int32)
    check(q.lib.kg_ft8_push(q.h, ptr(conns), 1, ptr(ncb), F.NS, ptr(bad), bad.size, ptr(np.ascontiguousarray(t)), t.size, ptr(ev), max_events, C.byref(ne), ptr(sl),
                            max_slots, C.byref(nsl)), "kg_ft8_push")
    assert ne.value == 3 and nsl.value == 1 and sl[0]["conn"] == 1 and sl[0]["num_blocks"] == F.SIZES[p]["slot_blocks"]
    assert (ev[ne.value:].view(np.uint8) == FILL).all() and (sl[nsl.value:].view(np.uint8) == FILL).all()        # behind the counts: the caller's
    assert first_difference(beside, freeze([tree(q, c) for c in (0, 2)])) is None
    assert live_allocs() == allocs
    info, lf, mag = q.state(1)
    last = q.state(1, previous=True)[2]
    assert info["num_blocks"] >= 3 and last.shape[0] == F.SIZES[p]["slot_blocks"] and last.max() > 200 and np.isfinite(sl[0]["max_mag"])      # and the connection did take them
    # the object goes on: after a new init a clean slot is the clean slot of a fresh object
    q.init(1, p)
    ev1, sl1 = q.push([1], x[None], t[None])
    fresh = Ft8(ctx, nconn=1)
    fresh.init(0, p)
    ev2, sl2 = fresh.push([0], x[None], t[None])
    sl1["conn"] = 0
    assert sl1.tobytes() == sl2.tobytes() and first_difference(freeze(tree(q, 1)[1:]), freeze(tree(fresh, 0)[1:])) is None
    fresh.close()
    q.close()
    ctx.close()
