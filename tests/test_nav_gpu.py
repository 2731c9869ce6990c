"""kg_nav on the GPU against the reference's records (tests/golden/nav_ref.npz) and the model (tests/nav_model.py): equality in every
field and byte, no tolerance anywhere."""
import numpy as np
import pytest

from flydog_sdr_gps_amd import KiwiGpuError, nav, trk
from . import nav_model as nm
from . import trk_common as tc
from .test_nav_cpu import CUTS, load_golden, same_frames, same_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def batches(golden, size=nav.MAX_CHANS):
    names = list(golden)
    return [names[a:a + size] for a in range(0, len(names), size)]


def check_states(ns, models, what):
    for ch, c in enumerate(models):
        same_state(ns.state(ch), c.state(), (what, ch))


def run_rounds(ctx, streams, sizes_of):
    """streams: [(mode, bits)] -> one NavSync channel each; round r pushes sizes_of(r, ch) bits of channel ch (0 allowed) until every
    stream is used up; the model runs beside it and kg_nav_get_state is compared with it after every push -> [frames per channel]"""
    ns = nav.NavSync(ctx, len(streams), [m for m, _ in streams])
    models = [nm.Channel(m) for m, _ in streams]
    got = [[] for _ in streams]
    at = [0] * len(streams)
    try:
        r = 0
        while any(a < b.size for a, (_, b) in zip(at, streams)):
            pieces = []
            for ch, (_, b) in enumerate(streams):
                n = min(sizes_of(r, ch), b.size - at[ch])
                pieces.append(b[at[ch]:at[ch] + n])
                at[ch] += n
            out = ns.push(pieces)
            for ch, p in enumerate(pieces):
                want = nm.frames(models[ch].push(p))
                same_frames(out[ch], want, ("round %d channel %d" % (r, ch)))
                got[ch].append(out[ch])
            check_states(ns, models, "round %d" % r)
            r += 1
            assert r < 5000
        check_states(ns, models, "end")
    finally:
        ns.close()
    return [np.concatenate(g) if g else np.zeros(0, nav.frame_dtype) for g in got]


def test_golden_in_one_push(gpu_ctx, golden):
    for names in batches(golden):
        streams = [(golden[n]["mode"], golden[n]["bits"]) for n in names]
        out = run_rounds(gpu_ctx, streams, lambda r, ch: 1 << 20)
        for n, fr in zip(names, out):
            same_frames(fr, golden[n]["frames"], n)


@pytest.mark.parametrize("which", range(4))
def test_golden_in_cuts(gpu_ctx, golden, which):
    """pushes of 16, 17, 299 / 499 and 301 / 501 bits"""
    for names in batches(golden):
        streams = [(golden[n]["mode"], golden[n]["bits"]) for n in names]
        out = run_rounds(gpu_ctx, streams, lambda r, ch: CUTS[streams[ch][0]][which][0])
        for n, fr in zip(names, out):
            same_frames(fr, golden[n]["frames"], (n, which))


@pytest.mark.parametrize("batch", range(3))
def test_pushes_of_one_bit(gpu_ctx, golden, batch):
    """every golden stream bit by bit, twelve channels at a time"""
    names = batches(golden)[batch]
    out = run_rounds(gpu_ctx, [(golden[n]["mode"], golden[n]["bits"]) for n in names], lambda r, ch: 1)
    for n, fr in zip(names, out):
        same_frames(fr, golden[n]["frames"], n)


def test_the_batches_hold_every_golden_stream(golden):
    assert len(batches(golden)) == 3 and sum(len(b) for b in batches(golden)) == len(golden)


def test_twelve_mixed_channels_unequal_pushes(gpu_ctx, golden):
    names = ["ca_random_2", "e1b_bursts", "ca_back_to_back_preambles", "e1b_word5_health", "ca_short", "e1b_short", "ca_swallowed_start",
             "e1b_chance_pair_in_page", "ca_flip_between", "e1b_all_zero_all_one", "ca_bit_error_w9", "e1b_alert"]
    sizes = (0, 1, 16, 301, 0, 17, 499, 501, 300, 2, 500, 0, 33)
    out = run_rounds(gpu_ctx, [(golden[n]["mode"], golden[n]["bits"]) for n in names], lambda r, ch: sizes[(r + 5 * ch) % len(sizes)])
    for n, fr in zip(names, out):
        same_frames(fr, golden[n]["frames"], n)
    assert sum(len(f) for f in out) > 60


def test_set_mode_in_mid_stream_restarts_the_channel(gpu_ctx, golden):
    a, b = golden["ca_leading_random"], golden["e1b_inverted"]
    ns = nav.NavSync(gpu_ctx, 2, [nav.L1, nav.E1B])
    try:
        before = ns.push([a["bits"][:777], b["bits"][:1234]])
        assert ns.state(0)["pushed"] == 777 and ns.state(1)["pushed"] == 1234
        ns.set_mode(0, nav.E1B)                        # channel 0 becomes E1B, channel 1 stays what it was
        st = ns.state(0)
        assert (st["holding"], st["bit0"], st["pushed"], st["held"].size) == (0, 0, 0, 0)
        out = ns.push([b["bits"], b["bits"][1234:]])
        same_frames(out[0], b["frames"], "restarted")
        same_frames(np.concatenate([before[1], out[1]]), b["frames"], "untouched")
        assert (ns.state(0)["holding"], ns.state(0)["bit0"]) == b["hold"]
    finally:
        ns.close()


def test_refusals_change_nothing(gpu_ctx, golden):
    a, b = golden["ca_back_to_back_preambles"], golden["e1b_upright"]
    ns = nav.NavSync(gpu_ctx, 2, [nav.L1, nav.E1B])
    models = [nm.Channel(nav.L1), nm.Channel(nav.E1B)]
    try:
        first = [a["bits"][:500], b["bits"][:700]]
        ns.push(first)
        for c, p in zip(models, first):
            c.push(p)
        rest = [a["bits"][500:], b["bits"][700:]]
        need = nav.cap_for(ns.modes, [r.size for r in rest])
        assert need == max(-(-rest[0].size // 30), -(-rest[1].size // 250)) and need > 1
        refused = []
        for call in (lambda: ns.push(rest, cap=need - 1),                       # cap below the bound
                     lambda: ns.push([rest[0], np.zeros(nav.MAX_PUSH + 1, np.uint8)]),
                     lambda: ns.set_mode(2, nav.L1), lambda: ns.set_mode(-1, nav.L1),        # bad channel
                     lambda: ns.set_mode(0, 2), lambda: ns.set_mode(1, -1)):                # bad mode
            with pytest.raises(KiwiGpuError) as e:
                call()
            refused.append(e.value.status)
            check_states(ns, models, "after a refusal")
        assert refused == [-2] * 6
        ns.modes = [nav.L1, nav.E1B]
        out = ns.push(rest, cap=need)
        for ch in range(2):
            same_frames(out[ch], nm.frames(models[ch].push(rest[ch])), "after the refusals")
        check_states(ns, models, "end")
    finally:
        ns.close()


# ---- epoch rows
class DevRows:
    """rows of kg_trk_epoch on the device with their counts, and the output buffers of a push"""

    def __init__(self, ctx, nchan, epoch_cap, cap):
        self.ctx, self.nchan, self.epoch_cap, self.cap = ctx, nchan, epoch_cap, cap
        self.d_ep = ctx.alloc(nchan * epoch_cap * trk.epoch_dtype.itemsize)
        self.d_cnt_in = ctx.alloc(4 * nchan)
        self.d_fr = ctx.alloc(nchan * max(cap, 1) * 64)
        self.d_cnt = ctx.alloc(4 * nchan)

    def free(self):
        for p in (self.d_ep, self.d_cnt_in, self.d_fr, self.d_cnt):
            self.ctx.free(p)

    def fetch(self):
        self.ctx.sync()
        counts = np.zeros(self.nchan, np.int32)
        self.ctx.download(self.d_cnt, counts)
        fr = np.zeros((self.nchan, max(self.cap, 1)), nav.frame_dtype)
        self.ctx.download(self.d_fr, fr)
        return [fr[ch, :counts[ch]].copy() for ch in range(self.nchan)]


def test_push_epochs_against_the_models_nav_bit_machine(gpu_ctx, golden):
    """synthetic kg_trk_epoch rows with only `flags` set (the other fields hold noise): C/A bits of 20 epochs with glitches and runs
    that break the 19-count, E1B saving every epoch, a negative count from a stopped channel, counts of 0"""
    rng = np.random.default_rng(8)
    ca = np.repeat(golden["ca_upright"]["bits"], 20)
    ca[rng.choice(ca.size, 60, replace=False)] ^= 1                             # glitches: most leave the bit, some restart the count
    e1 = golden["e1b_symbol_errors"]["bits"]
    flags = [ca, e1, np.repeat(golden["ca_inverted"]["bits"], 20)[5:]]
    modes = [nav.L1, nav.E1B, nav.L1]
    calls = ((3000, 700, 1), (0, 1, 8000), (21680, 1863, -1 - 6000), (60, 0, 0))       # records per channel and call
    epoch_cap = 21740
    cap = nav.cap_for_epochs(modes, epoch_cap)
    ns = nav.NavSync(gpu_ctx, 3, modes)
    models = [nm.Channel(m) for m in modes]
    dev = DevRows(gpu_ctx, 3, epoch_cap, cap)
    at = [0, 0, 0]
    nframes = 0
    try:
        for counts in calls:
            rows = np.zeros((3, epoch_cap), trk.epoch_dtype)
            rows.view(np.uint8)[:] = rng.integers(0, 256, rows.nbytes, dtype=np.uint8).reshape(rows.view(np.uint8).shape)
            want = []
            for ch, cnt in enumerate(counts):
                n = cnt if cnt >= 0 else -1 - cnt
                f = flags[ch][at[ch]:at[ch] + n]
                assert f.size == n
                at[ch] += n
                keep = rows["flags"][ch, :n] & ~np.uint32(trk.INAV)
                rows["flags"][ch, :n] = keep | (f.astype(np.uint32) * trk.INAV)
                want.append(nm.frames(models[ch].push(models[ch].nav_bits(f))))
            gpu_ctx.upload(dev.d_ep, rows)
            gpu_ctx.upload(dev.d_cnt_in, np.array(counts, np.int32))
            ns.push_epochs_dev(dev.d_ep, epoch_cap, dev.d_cnt_in, epoch_cap, dev.d_fr, max(cap, 1), cap, dev.d_cnt)
            got = dev.fetch()
            for ch in range(3):
                same_frames(got[ch], want[ch], ("epochs", counts, ch))
                nframes += len(got[ch])
            check_states(ns, models, counts)
        assert models[0].nav_glitch > 10 and nframes >= 6 and models[1].pushed == 2564
        with pytest.raises(KiwiGpuError):                                       # cap below the bound: refused, nothing changes
            ns.push_epochs_dev(dev.d_ep, epoch_cap, dev.d_cnt_in, epoch_cap, dev.d_fr, max(cap, 1), cap - 1, dev.d_cnt)
        check_states(ns, models, "after the refusal")
    finally:
        dev.free()
        ns.close()


def test_tracker_rows_straight_into_frame_sync(gpu_ctx):
    """the 130-nav-bit E1B scenario of tests/trk_common.py through kg_trk_process_bits_dev and, on the same device rows and counts,
    kg_nav_push_epochs_dev: the held bits are the firmware ring's"""
    sc = tc.scenarios()["e1b_nav130"]
    t = trk.Tracker(gpu_ctx, 1, sc.lo_delay, sc.cg_delay)
    ns = nav.NavSync(gpu_ctx, 1, [nav.E1B])
    n = sc.nclocks
    epoch_cap = trk.cap_for(n)
    cap = nav.cap_for_epochs([nav.E1B], epoch_cap)
    dev = DevRows(gpu_ctx, 1, epoch_cap, cap)
    d_bits = gpu_ctx.alloc(sc.bits.size)
    try:
        for s in sc.steps:
            op = s[0]
            if op == "S":
                t.set_sat(s[1], s[2])
            elif op == "C":
                t.set_e1b_code(s[1], sc.codes[s[2]])
            elif op == "G":
                t.set_rate_cg(s[1], s[2])
            elif op == "L":
                t.set_rate_lo(s[1], s[2])
            elif op == "l":
                t.set_gain_lo(s[1], s[2], s[3])
            elif op == "g":
                t.set_gain_cg(s[1], s[2], s[3])
            elif op == "R":
                t.sampler_reset()
            elif op == "X":
                gpu_ctx.upload(d_bits, sc.bits)
                t.process_dev(d_bits, n, dev.d_ep, epoch_cap, epoch_cap, dev.d_cnt_in)
                ns.push_epochs_dev(dev.d_ep, epoch_cap, dev.d_cnt_in, epoch_cap, dev.d_fr, max(cap, 1), cap, dev.d_cnt)
            else:
                assert op == "D", op
        frames = dev.fetch()[0]
        count = np.zeros(1, np.int32)
        gpu_ctx.download(dev.d_cnt_in, count)
        st = ns.state(0)
        assert count[0] >= 130 and st["pushed"] == count[0] and st["holding"] == count[0] - sum(int(f["consumed"]) for f in frames)
        assert len(frames) == 0 and st["holding"] >= 112       # noise holds no preamble pair here; every bit is still held
        assert np.array_equal(st["held"][-112:], trk.nav_bits_of(t.get_chan(0), 112))
    finally:
        gpu_ctx.free(d_bits)
        dev.free()
        ns.close()
        t.close()
