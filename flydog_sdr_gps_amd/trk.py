"""GPS tracking channels over the C ABI (kg_trk): what receives the words of handoff.chan_start.

Reference                                                                 here
  DEMOD x 12, the pause counter       verilog/gps/demod.v, gps.v:190-263 -> Tracker.process / process_dev
  GPS_Method, CloseLoop               e_cpu/kiwi.gps.asm:57-449          -> (inside the kernel, once per epoch)
  CmdSetSat / SetRate / set_gain ...  e_cpu/kiwi.gps.asm:482-593         -> Tracker.set_sat / set_rate_lo ...
  CHANNEL::Reset / Start              gps/channel.cpp:200-321            -> Tracker.reset_channel / start_channel
  struct UPLOAD                       gps/channel.cpp:38-52              -> chan_dtype, Tracker.get_chan

scene_bits() is an input generator (numpy), not part of the measured path.
"""
import ctypes as C

import numpy as np

from . import sats as _sats
from ._lib import Context, check, ptr  # noqa: F401

MAX_CHANS = 12
E1B_MODE, G2_INIT = 0x800, 0x400
CHAN_BYTES = 78
MAX_NAV_BITS = 128
LO_DELAY, CG_DELAY = 216, 577
MIN_EPOCH = 8184
UNLOCKED, INAV = 1, 2
FS, FC, CPS = 16.368e6, 4.092e6, 1.023e6               # gps/gps.h:42-46

epoch_dtype = np.dtype([("clock", "<u8"), ("ip", "<i4"), ("qp", "<i4"), ("ie", "<i4"), ("qe", "<i4"), ("il", "<i4"), ("ql", "<i4"),
                        ("lo_rate", "<u4"), ("cg_rate", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
# struct UPLOAD of gps/channel.cpp (== STRUCT GPS_CHAN of kiwi.gps.asm)
chan_dtype = np.dtype([("nav_ms", "<u2"), ("nav_bits", "<u2"), ("nav_glitch", "<u2"), ("nav_prev", "<u2"), ("nav_buf", "<u2", (MAX_NAV_BITS // 16,)),
                       ("ca_freq", "<u8"), ("lo_freq", "<u8"), ("iq", "<u2", (3, 4)), ("ca_gain", "<u2", (2,)), ("lo_gain", "<u2", (2,)),
                       ("ca_unlocked", "<u2"), ("E1B_mode", "<u2"), ("LO_polarity", "<u2")])
assert epoch_dtype.itemsize == 48 and chan_dtype.itemsize == CHAN_BYTES


def codegen_init(sat):
    """the CmdSetSat word of row `sat` of sats.SATS (gps/search.cpp:556-563)"""
    prn, t1, t2, kind = _sats.SATS[sat]
    if kind == _sats.E1B:
        return E1B_MODE | (prn - 1)
    if kind == _sats.QZSS:
        return G2_INIT | t2
    return (t1 << 4) + t2


def gains(is_e1b, adj_lo=0, adj_cg=0):
    """-> ((lo_ki, lo_kp - lo_ki), (cg_ki, cg_kp - cg_ki)) of CHANNEL::SetGainAdjLO / SetGainAdjCG (gps/channel.cpp:170-196)"""
    e = -3 if is_e1b else 0
    return (20 + e + adj_lo, 7), (11 + adj_cg, 12)


def cap_for(nclocks):
    return int(nclocks) // MIN_EPOCH + 2


class Tracker:
    """A bank of nchan tracking channels on the GPU (kg_trk)."""

    def __init__(self, ctx=None, nchan=MAX_CHANS, lo_delay=0, cg_delay=0, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self.lib = self.ctx.lib
        self.nchan = int(nchan)
        h = C.c_void_p()
        check(self.lib.kg_trk_create(self.ctx.h, int(nchan), int(lo_delay), int(cg_delay), C.byref(h)), "kg_trk_create")
        self.h = h
        self.stopped = []

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):
                self.lib.kg_trk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_sat(self, ch, word):
        check(self.lib.kg_trk_set_sat(self.h, int(ch), int(word)), "kg_trk_set_sat")

    def set_e1b_code(self, ch, chips):
        chips = np.ascontiguousarray(chips, np.uint8)
        check(self.lib.kg_trk_set_e1b_code(self.h, int(ch), ptr(chips), int(chips.size)), "kg_trk_set_e1b_code")

    def set_rate_lo(self, ch, rate):
        check(self.lib.kg_trk_set_rate_lo(self.h, int(ch), int(rate) & 0xFFFFFFFF), "kg_trk_set_rate_lo")

    def set_rate_cg(self, ch, rate):
        check(self.lib.kg_trk_set_rate_cg(self.h, int(ch), int(rate) & 0xFFFFFFFF), "kg_trk_set_rate_cg")

    def set_gain_lo(self, ch, ki, kp_minus_ki):
        check(self.lib.kg_trk_set_gain_lo(self.h, int(ch), int(ki), int(kp_minus_ki)), "kg_trk_set_gain_lo")

    def set_gain_cg(self, ch, ki, kp_minus_ki):
        check(self.lib.kg_trk_set_gain_cg(self.h, int(ch), int(ki), int(kp_minus_ki)), "kg_trk_set_gain_cg")

    def set_polarity(self, ch, pol):
        check(self.lib.kg_trk_set_polarity(self.h, int(ch), int(pol)), "kg_trk_set_polarity")

    def set_mask(self, mask):
        check(self.lib.kg_trk_set_mask(self.h, int(mask) & 0xFFFFFFFF), "kg_trk_set_mask")

    def sampler_reset(self):
        check(self.lib.kg_trk_sampler_reset(self.h), "kg_trk_sampler_reset")

    def pause(self, ch, count):
        check(self.lib.kg_trk_pause(self.h, int(ch), int(count)), "kg_trk_pause")

    def set_loop(self, ch, on):
        check(self.lib.kg_trk_set_loop(self.h, int(ch), int(bool(on))), "kg_trk_set_loop")

    def reset_channel(self, ch, sat, e1b_chips=None):
        """CHANNEL::Reset: the satellite, the E1B code, the nominal code rate, the gains"""
        word = codegen_init(sat)
        self.set_sat(ch, word)
        if word & E1B_MODE:
            self.set_e1b_code(ch, e1b_chips)
        self.set_rate_cg(ch, int(CPS / FS * 2.0 ** 32))
        lo, cg = gains(bool(word & E1B_MODE))
        self.set_gain_cg(ch, *cg)
        self.set_gain_lo(ch, *lo)

    def start_channel(self, ch, start):
        """CHANNEL::Start with a handoff.ChanStart: the two rates, then the pause that lines the code up"""
        self.set_rate_lo(ch, start.lo_rate)
        self.set_rate_cg(ch, start.ca_rate)
        if start.ca_pause:
            self.pause(ch, start.ca_pause - 1)

    def process_dev(self, d_bits, nclocks, d_epochs, chan_stride, cap, d_counts):
        """enqueue only; every pointer is a device address (int)"""
        check(self.lib.kg_trk_process_bits_dev(self.h, C.c_void_p(int(d_bits)), int(nclocks), C.c_void_p(int(d_epochs)), int(chan_stride),
                                               int(cap), C.c_void_p(int(d_counts))), "kg_trk_process_bits_dev")

    def process(self, bits, nclocks):
        """bits: the bytes from the one that holds the next bit on -> [epoch_dtype array per channel]; self.stopped lists the channels
        whose code loop wrote a word outside the accepted range and which stand since (set_rate_cg starts one again)"""
        bits = np.ascontiguousarray(bits, np.uint8)
        cap = cap_for(nclocks)
        ep = np.zeros((self.nchan, cap), epoch_dtype)
        counts = np.zeros(self.nchan, np.int32)
        check(self.lib.kg_trk_process_bits(self.h, ptr(bits), int(nclocks), ptr(ep), cap, cap, ptr(counts)), "kg_trk_process_bits")
        self.stopped = [ch for ch in range(self.nchan) if counts[ch] < 0]       # count -1 - n: the code loop left [2^27, 2^29)
        return [ep[ch, :(counts[ch] if counts[ch] >= 0 else -1 - counts[ch])].copy() for ch in range(self.nchan)]

    def get_chan(self, ch):
        """-> the GPS_CHAN record (a chan_dtype scalar)"""
        out = np.zeros(CHAN_BYTES, np.uint8)
        check(self.lib.kg_trk_get_chan(self.h, int(ch), ptr(out)), "kg_trk_get_chan")
        return out.view(chan_dtype)[0]

    def get_clocks(self):
        """-> (clocks consumed, the 18-bit replica word of every channel)"""
        clock = C.c_uint64()
        rep = np.zeros(self.nchan, np.uint32)
        check(self.lib.kg_trk_get_clocks(self.h, C.byref(clock), ptr(rep)), "kg_trk_get_clocks")
        return clock.value, rep


def nav_bits_of(chan, nbits):
    """the last nbits (<= 112) nav bits of a GPS_CHAN record, oldest first.  ch_NAV_BUF is a ring of 16-bit words and ch_NAV_BITS
    the write position; NavSave shifts a word left and adds the bit, so a word holds its first bit highest: bit 15 once it is full,
    bit (count - 1) while only `count` of its bits are written."""
    wr = int(chan["nav_bits"])
    buf = [int(w) for w in chan["nav_buf"]]
    out = []
    for k in range(nbits, 0, -1):
        pos = (wr - k) % MAX_NAV_BITS                   # the bit written k services ago
        word, in_word = pos // 16, pos % 16
        count = wr % 16 if (word == wr // 16 and wr % 16) else 16
        out.append((buf[word] >> (count - 1 - in_word)) & 1)
    return np.array(out, np.uint8)


def scene_bits(chips, n, code_phase, doppler_hz, cn0_dbhz, data_bits, seed, theta=0.7, boc=False, bit_epochs=20, flips=()):
    """A packed 1-bit IF stream of n clocks holding ONE satellite: code `chips` (0/1) starting `code_phase` chips into its epoch at
    clock 0, carrier FC + doppler_hz with the code rate following it (CPS (1 + doppler / L1)), 50 bps data (data_bits, 0/1, one per
    bit_epochs code epochs, aligned to the code epoch at clock 0 minus code_phase), white noise for cn0_dbhz.  flips: clock indices
    from which on the data sign is inverted once more (a mid-bit flip).  bit = x < 0, LSB first (synth.gps_scene_bits' convention)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    chips = np.asarray(chips, np.uint8)
    out = np.empty((n + 7) // 8, np.uint8)
    a = np.sqrt(4.0 * 10.0 ** (cn0_dbhz / 10.0) / FS)
    rate = CPS * (1.0 + doppler_hz / 1575.42e6) / FS    # chips per clock
    block = 1 << 20
    data_bits = np.asarray(data_bits, np.int64)
    for s in range(0, n, block):
        m = min(block, n - s)
        t = np.arange(s, s + m, dtype=np.float64)
        pos = t * rate + code_phase                     # chips since the epoch start before clock 0
        idx = np.floor(pos).astype(np.int64)
        code = 1.0 - 2.0 * chips[idx % chips.size]
        if boc:
            code = code * np.where(pos - idx >= 0.5, -1.0, 1.0)
        nbit = (idx // chips.size) // bit_epochs
        d = 1.0 - 2.0 * data_bits[nbit % data_bits.size]
        for f in flips:
            d = np.where(t >= f, -d, d)
        x = rng.standard_normal(m) + a * d * code * np.cos(2 * np.pi * ((FC + doppler_hz) / FS) * t + theta)
        b = (x < 0).astype(np.uint8)
        if m % 8:
            b = np.concatenate([b, np.zeros(8 - m % 8, np.uint8)])
        out[s // 8:s // 8 + b.size // 8] = np.packbits(b, bitorder="little")
    return out
