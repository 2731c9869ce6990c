"""kg_eph on the GPU against the reference's records (tests/golden/eph_ref.npz) and the model (tests/eph_model.py): decoded state,
channel state, UTC fields and notes equal in every bit; position and clock within the bars derived in tests/test_eph_cpu.py."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import KiwiGpuError, eph, nav
from . import eph_model as em
from . import nav_model as nm
from .test_eph_cpu import REFUSED, check_sv, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def segments(ev):
    """the events cut where a bind follows frames -> [(binds [(ch, sat, kind)], frames {ch: [index]}, the frame indices in event order)]"""
    out, binds, rows, order = [], [], {}, []
    for op, ch, a, b in ev:
        if op == 0:
            if order:
                out.append((binds, rows, order))
                binds, rows, order = [], {}, []
            binds.append((int(ch), int(a), int(b)))
        else:
            rows.setdefault(int(ch), []).append(int(a))
            order.append(int(a))
    out.append((binds, rows, order))
    return out


def push(e, frames, rows):
    """rows: {ch: [frame index]} -> {index: note}"""
    notes = e.push_frames([frames[rows.get(ch, [])] for ch in range(e.nchan)])
    return {a: notes[ch][k] for ch, idx in rows.items() for k, a in enumerate(idx)}


def check_after(e, s, sat_of, rows, last, what, utc=True):
    """the satellites and channels of `rows` against the reference's records after each one's last frame; UTC after frame `last`"""
    for ch, idx in rows.items():
        a = idx[-1]
        assert e.get(sat_of[ch]).tobytes() == s["eph"][a].tobytes(), (what, "kg_ephem of channel %d after frame %d" % (ch, a))
        c = e.chan(ch)
        assert (c["sat"], c["week_gst"], c["toes"], c["toc_gst"]) == (sat_of[ch],) + tuple(int(v) for v in s["chan"][a]), (what, ch, a, c)
    if utc:
        u = e.utc()
        assert (u["delta_tLS"], u["delta_tLSF"], u["tLS_valid"]) == tuple(int(v) for v in s["utc"][last]), (what, last, u)


def run_scenario(ctx, s, single, what, ch_off=0, e=None):
    own = e is None
    e = eph.Ephemerides(ctx, 12) if own else e
    try:
        sat_of = {}
        for binds, rows, order in segments(s["ev"]):
            for ch, sat, kind in binds:
                e.set_sat(ch + ch_off, sat, kind)
                sat_of[ch + ch_off] = sat
            rows = {ch + ch_off: idx for ch, idx in rows.items()}
            if single:                                                  # one frame per push, in the reference's order
                ch_of = {a: ch for ch, idx in rows.items() for a in idx}
                for a in order:
                    got = push(e, s["frames"], {ch_of[a]: [a]})
                    assert got[a].tobytes() == s["notes"][a].tobytes(), (what, "note", a, got[a], s["notes"][a])
                    check_after(e, s, sat_of, {ch_of[a]: [a]}, a, what, utc=own)
            else:
                got = push(e, s["frames"], rows)
                for a in order:
                    assert got[a].tobytes() == s["notes"][a].tobytes(), (what, "note", a, got[a], s["notes"][a])
                check_after(e, s, sat_of, rows, order[-1], what, utc=own)
        return e
    finally:
        if own:
            e.close()


@pytest.mark.parametrize("single", (False, True))
def test_golden_streams(gpu_ctx, golden, single):
    """every golden scenario pushed whole and one frame per push: cutting must not matter"""
    for name, s in golden.items():
        run_scenario(gpu_ctx, s, single, (name, "single" if single else "whole"))


def test_twelve_channels_mixed(gpu_ctx, golden):
    """C/A channels 0..6 and E1B channels 7..11 of ONE object against the records of the scenarios run apart"""
    ca, gal = golden["ca"], golden["gal"]
    ca7 = dict(ca, ev=np.array([v for v in ca["ev"] if v[1] < 7]))
    e = eph.Ephemerides(gpu_ctx, 12)
    try:
        run_scenario(gpu_ctx, ca7, False, "mixed ca", 0, e)
        run_scenario(gpu_ctx, gal, False, "mixed gal", 7, e)
        for sat, want in list(final(ca7).items()) + list(final(gal).items()):
            assert e.get(sat).tobytes() == want.tobytes(), sat
        last_ca = [a for op, ch, a, b in ca7["ev"] if op == 1][-1]
        u = e.utc()
        assert (u["delta_tLS"], u["delta_tLSF"], u["tLS_valid"]) == tuple(int(v) for v in ca["utc"][last_ca]) and u["tLS_valid"] == 1
    finally:
        e.close()
    # and truly at once: the first segment of both in ONE push
    e = eph.Ephemerides(gpu_ctx, 12)
    try:
        rows, sat_of = {}, {}
        for s, off in ((ca7, 0), (gal, 7)):
            binds, r, _ = segments(s["ev"])[0]
            for ch, sat, kind in binds:
                e.set_sat(ch + off, sat, kind)
                sat_of[ch + off] = sat
            rows.update({ch + off: (s, idx) for ch, idx in r.items()})
        assert len(rows) == 12
        notes = e.push_frames([rows[ch][0]["frames"][rows[ch][1]] for ch in range(12)])
        for ch, (s, idx) in rows.items():
            assert notes[ch].tobytes() == s["notes"][idx].tobytes(), ch
            assert e.get(sat_of[ch]).tobytes() == s["eph"][idx[-1]].tobytes(), ch
    finally:
        e.close()


def final(s):
    sat_of, out = {}, {}
    for op, ch, a, b in s["ev"]:
        if op == 0:
            sat_of[ch] = a
        else:
            out[sat_of[ch]] = s["eph"][a]
    return out


def chained_subframes(rng, subs):
    """C/A subframes with random raw fields whose parity chain ends every subframe at D29 = D30 = 0 -> 300 bits each"""
    out, d29, d30 = [], 0, 0
    for k, sub in enumerate(subs):
        fields = {name: int(rng.integers(0, 1 << n)) for name, (_, n) in eph.L1_FIELDS[sub].items()}
        if sub == 4:
            fields["page"] = eph.PAGE18
        while True:
            f = nav.l1_subframe(eph.subframe_words(sub, fields, tow=1000 + k, fill=rng.integers(0, 2, 240)), d29, d30)
            if not f[-2] and not f[-1]:
                break
        d29, d30 = int(f[-2]), int(f[-1])
        out.append(f)
    return out


def test_bits_to_ephemeris_on_the_device(gpu_ctx):
    """NavSync's rows and counts fed straight into push_frames_dev: one C/A stream of 5 subframes, one E1B stream of 6 pages"""
    rng = np.random.default_rng(31)
    ca_bits = np.concatenate([rng.integers(0, 2, 13).astype(np.uint8)] + chained_subframes(rng, (1, 2, 3, 4, 5)) + [rng.integers(0, 2, 40).astype(np.uint8)])
    pages = []
    for wt in (5, 1, 2, 3, 4, 10):
        fields = {name: int(rng.integers(0, 1 << n)) for name, (_, n) in eph.INAV_FIELDS[wt].items()}
        if wt == 5:
            fields.update(e1bhs=0, e1bdvs=0, week=1301)
        pages.append(nav.e1b_page(eph.inav_word(wt, fields, fill=rng.integers(0, 2, 128)), reserved=rng.integers(0, 2, 64)))
    e1_bits = np.concatenate(pages + [rng.integers(0, 2, 30).astype(np.uint8)])
    streams, modes = [ca_bits, e1_bits], [nav.L1, nav.E1B]
    model = em.Model(2)
    model.set_sat(0, 5, eph.NAVSTAR)
    model.set_sat(1, 33, eph.E1B)
    want = [[model.push(ch, f) for f in nm.run(modes[ch], streams[ch])[0]] for ch in range(2)]
    assert [len(w) for w in want] == [5, 6] and all(n["applied"] for w in want for n in w)

    ctx = gpu_ctx
    nb = np.array([b.size for b in streams], np.int32)
    stride = int(nb.max())
    cap = nav.cap_for(modes, nb)
    host = np.zeros((2, stride), np.uint8)
    for ch, b in enumerate(streams):
        host[ch, :b.size] = b
    d_bits, d_fr, d_cnt, d_no = ctx.alloc(host.nbytes), ctx.alloc(2 * cap * 64), ctx.alloc(8), ctx.alloc(2 * cap * 32)
    ns, e = nav.NavSync(ctx, 2, modes), eph.Ephemerides(ctx, 2)
    try:
        ctx.upload(d_bits, host)
        e.set_sat(0, 5, eph.NAVSTAR)
        e.set_sat(1, 33, eph.E1B)
        ns.push_dev(d_bits, stride, nb, d_fr, cap, cap, d_cnt)
        e.push_frames_dev(d_fr, cap, d_cnt, cap, d_no, cap)             # no host copy in between
        ctx.sync()
        counts, notes = np.zeros(2, np.int32), np.zeros((2, cap), eph.note_dtype)
        ctx.download(d_cnt, counts)
        ctx.download(d_no, notes)
        assert counts.tolist() == [5, 6]
        for ch in range(2):
            assert notes[ch, :counts[ch]].tobytes() == b"".join(n.tobytes() for n in want[ch]), ch
        assert e.get(5).tobytes() == model.slot[5].tobytes() and e.get(33).tobytes() == model.slot[33].tobytes()
        assert e.get(5)["valid"] == model.valid(model.slot[5]) and e.utc() == model.utc and model.utc["tLS_valid"] == 1
        c = e.chan(1)
        assert (c["week_gst"], c["toes"], c["toc_gst"]) == (1301, model.chan[1]["toes"], model.chan[1]["toc_gst"])
    finally:
        ns.close()
        e.close()
        for p in (d_bits, d_fr, d_cnt, d_no):
            ctx.free(p)


def test_counts_and_error_rows(gpu_ctx, golden):
    """counts of 0, 1 and cap in one push, and a row of frames that must not be applied"""
    ca, gal = golden["ca"], golden["gal"]
    rows = segments(ca["ev"])[0][1]
    errs = gal["frames"][np.isin(gal["frames"]["err"], (nav.ERR_SLIP, nav.ERR_CRC, nav.ERR_ALERT))]
    assert len(errs) >= 4
    e = eph.Ephemerides(gpu_ctx, 4)
    try:
        for ch, (sat, kind) in enumerate(((0, eph.NAVSTAR), (1, eph.NAVSTAR), (2, eph.NAVSTAR), (40, eph.E1B))):
            e.set_sat(ch, sat, kind)
        full = ca["frames"][rows[1]]                                    # channel 1's seven frames: the cap
        notes = e.push_frames([ca["frames"][:0], ca["frames"][rows[2][:1]], full, errs])
        assert [len(n) for n in notes] == [0, 1, len(full), len(errs)]
        assert notes[1].tobytes() == ca["notes"][rows[2][:1]].tobytes() and notes[2].tobytes() == ca["notes"][rows[1]].tobytes()
        assert not notes[3]["applied"].any() and not notes[3]["tow_updated"].any()
        assert (notes[3]["bit_next"] == errs["bit"] + errs["consumed"].astype(np.uint64)).all()
        blank = np.zeros((), eph.ephem_dtype)
        blank["kind"] = eph.E1B
        assert e.get(40).tobytes() == blank.tobytes() and e.get(0).tobytes() == np.zeros((), eph.ephem_dtype).tobytes()
        assert e.get(2).tobytes() == ca["eph"][rows[1][-1]].tobytes() and e.chan(3)["week_gst"] == 0
        notes = e.push_frames([ca["frames"][:0]] * 4)                  # nothing at all
        assert all(len(n) == 0 for n in notes)
        par = ca["frames"][ca["frames"]["err"] == nav.ERR_PARITY]      # C/A parity failures only
        before = e.get(1).tobytes()
        notes = e.push_frames([par[:0], par, par[:0], par[:0]])
        assert not notes[1]["applied"].any() and e.get(1).tobytes() == before
    finally:
        e.close()


def test_set_sat_and_clear(gpu_ctx, golden):
    gal = golden["gal"]
    e = eph.Ephemerides(gpu_ctx, 3)
    try:
        e.set_sat(0, 20, eph.E1B)
        for args in ((1, 20, eph.E1B), (3, 1, eph.E1B), (0, 64, eph.E1B), (0, -2, eph.E1B), (0, 1, 3)):
            with pytest.raises(KiwiGpuError):
                e.set_sat(*args)
        e.set_sat(0, 20, eph.E1B)                                       # its own satellite again: fine
        with pytest.raises(KiwiGpuError):
            eph.Ephemerides(gpu_ctx, 13)
        rows = segments(gal["ev"])[0][1][0]                             # channel 0's first segment: ends with a week and a Valid sat 20
        e.push_frames([gal["frames"][rows], gal["frames"][:0], gal["frames"][:0]])
        week = e.chan(0)["week_gst"]
        assert week == int(gal["chan"][rows[-1]][0]) != 0 and e.get(20)["valid"] == 1
        # a rebind carries the week: words 1 and 4 alone give t_oe and t_oc
        e.set_sat(0, 25, eph.E1B)
        assert e.chan(0) == dict(sat=25, week_gst=week, toes=e.chan(0)["toes"], toc_gst=e.chan(0)["toc_gst"])
        seg = segments(gal["ev"])[1][1][0]
        e.push_frames([gal["frames"][seg], gal["frames"][:0], gal["frames"][:0]])
        got = e.get(25)
        assert got.tobytes() == gal["eph"][seg[-1]].tobytes() and got["t_oe"] != 0 and got["t_oc"] != 0 and got["valid"] == 1
        assert e.get(20)["valid"] == 1                                  # the slot left behind persists
        e.set_sat(1, 20, eph.E1B)                                       # and may now go to another channel
        # a kind change re-evaluates Valid: as C/A the slot's IODC is 0
        e.set_sat(1, 20, eph.CA)
        assert e.get(20)["valid"] == 0 and e.get(20)["kind"] == eph.CA
        e.set_sat(1, 20, eph.E1B)
        assert e.get(20)["valid"] == 1
        e.clear_chan(0)
        assert e.chan(0) == dict(sat=25, week_gst=0, toes=0, toc_gst=0)
        e.clear_sat(25)
        blank = np.zeros((), eph.ephem_dtype)
        blank["kind"] = eph.E1B
        assert e.get(25).tobytes() == blank.tobytes()
        e.set_sat(0, -1)
        notes = e.push_frames([gal["frames"][seg], gal["frames"][:0], gal["frames"][:0]])      # an unbound channel: read, not applied
        assert not notes[0]["applied"].any() and e.get(25).tobytes() == blank.tobytes() and e.chan(0)["sat"] == -1
        for call in (lambda: e.clear_sat(64), lambda: e.clear_chan(3), lambda: e.get(-1)):
            with pytest.raises(KiwiGpuError):
                call()
    finally:
        e.close()


@pytest.fixture(scope="module")
def loaded(gpu_ctx, golden):
    """one object per scenario with every stream pushed: shared by the snapshot tests, which only read it"""
    objs = {name: run_scenario(gpu_ctx, s, False, name, 0, eph.Ephemerides(gpu_ctx, 12)) for name, s in golden.items()}
    yield objs
    for e in objs.values():
        e.close()


def test_sv_full_set(loaded, golden):
    """every flag path; the measured maxima are printed (tools/eph_accuracy.py keeps them)"""
    for name, s in golden.items():
        poison = np.frombuffer(np.full(len(s["snaps"]) * eph.sv_dtype.itemsize, 0xA5, np.uint8).tobytes(), eph.sv_dtype).copy()
        got = loaded[name].sv(s["snaps"], out=poison.copy())
        stats = check_sv(got, s, name)
        print(name, stats)
        refused = (s["svi"][:, 0] & REFUSED) != 0
        assert refused.sum() >= 20 and set(s["svi"][refused, 0]) == {eph.SV_NOT_VALID, eph.SV_POWER}
        for f in ("x", "y", "z", "ct", "t_k", "week"):                  # a refused snapshot's row keeps its values, flags apart
            assert got[f][refused].tobytes() == poison[f][refused].tobytes(), (name, f)
        assert stats["n"] >= 100


@pytest.mark.parametrize("nsnap", (1, 63, 64, 65))
def test_sv_wave_edge(loaded, golden, nsnap):
    s = golden["ca"]
    full = loaded["ca"].sv(s["snaps"])
    for first in (0, 17):
        got = loaded["ca"].sv(s["snaps"][first:first + nsnap])
        assert got.tobytes() == full[first:first + nsnap].tobytes(), (nsnap, first)
    assert loaded["ca"].sv(s["snaps"][:0]).size == 0
