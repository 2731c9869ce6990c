"""Nav frame sync over the C ABI (kg_nav): what turns a tracking channel's nav bits into validated frames.

Reference                                                                 here
  the `holding` loop                  gps/channel.cpp:441-506            -> NavSync.push / push_dev / push_epochs_dev
  CHANNEL::ParityCheck, L1_parity     gps/channel.cpp:731-832, :125-135  -> (inside the kernels)
  E1B_subframe, checkcrc_e1b          gps/GNSS-SDRLIB/sdrnav_gal.cpp     -> (inside the kernels)
  the nav-bit machine                 e_cpu/kiwi.gps.asm NavSave         -> push_epochs_dev

Not here: Ephemeris[].Subframe, decode_word0..10, CHANNEL::Subframe, nav.tow_updated; probation, alert, abort, bits_tow and
expecting_preamble (host decisions on a record's id, err and bit); the gps_debug dropped-subframe simulation and TEST_VECTOR.

l1_subframe() and e1b_page() are ENCODERS (numpy): input generators for tests and synthetic scenes, not part of the measured path.
"""
import ctypes as C

import numpy as np

from ._lib import Context, check, ptr  # noqa: F401

L1, E1B = 0, 1
SUBFRAME_BITS = {L1: 300, E1B: 500}
MIN_RECORD_BITS = {L1: 30, E1B: 250}
ERR_SLIP, ERR_CRC, ERR_ALERT, ERR_OOS, ERR_PAGE, ERR_PARITY = 1, 2, 3, 4, 5, 16
MAX_PUSH, MAX_HELD, MAX_CHANS = 65536, 499, 12
L1_PREAMBLE = np.array([1, 0, 0, 0, 1, 0, 1, 1], np.uint8)
E1B_PREAMBLE = np.array([0, 1, 0, 1, 1, 0, 0, 0, 0, 0], np.uint8)

frame_dtype = np.dtype([("bit", "<u8"), ("err", "<i4"), ("consumed", "<i4"), ("inverted", "<i4"), ("id", "<i4"), ("data", "u1", (40,))])
assert frame_dtype.itemsize == 64


def cap_for(modes, nbits):
    """the smallest cap kg_nav_push_bits_dev accepts: ceil(nbits / 30) for a C/A channel, ceil(nbits / 250) for an E1B one"""
    return max([-(-int(n) // MIN_RECORD_BITS[m]) for m, n in zip(modes, nbits)] + [0])


def cap_for_epochs(modes, epoch_cap):
    return cap_for(modes, [int(epoch_cap) if m == E1B else -(-int(epoch_cap) // 20) for m in modes])


class NavSync:
    """nchan frame synchronisers on the GPU (kg_nav); modes: KG_NAV_L1 / KG_NAV_E1B per channel (default: all C/A)"""

    def __init__(self, ctx=None, nchan=MAX_CHANS, modes=None, device=0):
        self.ctx = ctx if ctx is not None else Context(device)
        self.lib = self.ctx.lib
        self.nchan = int(nchan)
        h = C.c_void_p()
        check(self.lib.kg_nav_create(self.ctx.h, int(nchan), C.byref(h)), "kg_nav_create")
        self.h = h
        self.modes = [L1] * self.nchan
        for ch, m in enumerate(modes or ()):
            self.set_mode(ch, m)

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):
                self.lib.kg_nav_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_mode(self, ch, mode):
        """empties the channel and restarts its stream index and its nav-bit machine"""
        check(self.lib.kg_nav_set_mode(self.h, int(ch), int(mode)), "kg_nav_set_mode")
        self.modes[ch] = int(mode)

    def push_dev(self, d_bits, chan_stride, nbits, d_frames, frame_stride, cap, d_counts):
        """enqueue only; nbits: one int per channel (host); the other pointers are device addresses (int)"""
        nb = np.ascontiguousarray(nbits, np.int32)
        assert nb.size == self.nchan
        check(self.lib.kg_nav_push_bits_dev(self.h, C.c_void_p(int(d_bits)), int(chan_stride), ptr(nb), C.c_void_p(int(d_frames)),
                                            int(frame_stride), int(cap), C.c_void_p(int(d_counts))), "kg_nav_push_bits_dev")

    def push_epochs_dev(self, d_epochs, chan_stride, d_counts_in, epoch_cap, d_frames, frame_stride, cap, d_counts):
        """enqueue only: the rows and counts of Tracker.process_dev (device addresses), epoch_cap that call's cap"""
        check(self.lib.kg_nav_push_epochs_dev(self.h, C.c_void_p(int(d_epochs)), int(chan_stride), C.c_void_p(int(d_counts_in)), int(epoch_cap),
                                              C.c_void_p(int(d_frames)), int(frame_stride), int(cap), C.c_void_p(int(d_counts))),
              "kg_nav_push_epochs_dev")

    def push(self, bits, cap=None):
        """bits: one array of 0 / 1 per channel (any may be empty) -> [frame_dtype array per channel]"""
        assert len(bits) == self.nchan
        rows = [np.ascontiguousarray(b, np.uint8).reshape(-1) for b in bits]
        nb = np.array([r.size for r in rows], np.int32)
        stride = max(int(nb.max()), 1)
        host = np.zeros((self.nchan, stride), np.uint8)
        for ch, r in enumerate(rows):
            host[ch, :r.size] = r
        cap = cap_for(self.modes, nb) if cap is None else int(cap)
        fr = np.zeros((self.nchan, max(cap, 1)), frame_dtype)
        counts = np.zeros(self.nchan, np.int32)
        check(self.lib.kg_nav_push_bits(self.h, ptr(host), stride, ptr(nb), ptr(fr), max(cap, 1), cap, ptr(counts)), "kg_nav_push_bits")
        return [fr[ch, :counts[ch]].copy() for ch in range(self.nchan)]

    def state(self, ch):
        """-> dict(holding, bit0, held (0 / 1 array), pushed, nav_ms, nav_prev, nav_glitch); synchronises"""
        holding, bit0, pushed = C.c_int32(), C.c_uint64(), C.c_uint64()
        held = np.zeros(MAX_HELD, np.uint8)
        nav3 = np.zeros(3, np.int32)
        check(self.lib.kg_nav_get_state(self.h, int(ch), C.byref(holding), C.byref(bit0), ptr(held), C.byref(pushed), ptr(nav3)), "kg_nav_get_state")
        return dict(holding=holding.value, bit0=bit0.value, held=held[:holding.value].copy(), pushed=pushed.value,
                    nav_ms=int(nav3[0]), nav_prev=int(nav3[1]), nav_glitch=int(nav3[2]))


# ---- encoders
# IS-GPS-200 table 20-XIV: the source data bits d1..d24 (1-based) under each parity bit D25..D30, and which of D29* / D30* it takes
_L1_EQ = (
    (29, (1, 2, 3, 5, 6, 10, 11, 12, 13, 14, 17, 18, 20, 23)),
    (30, (2, 3, 4, 6, 7, 11, 12, 13, 14, 15, 18, 19, 21, 24)),
    (29, (1, 3, 4, 5, 7, 8, 12, 13, 14, 15, 16, 19, 20, 22)),
    (30, (2, 4, 5, 6, 8, 9, 13, 14, 15, 16, 17, 20, 21, 23)),
    (30, (1, 3, 5, 6, 7, 9, 10, 14, 15, 16, 17, 18, 21, 22, 24)),
    (29, (3, 5, 6, 8, 9, 10, 11, 13, 15, 19, 22, 23, 24)),
)


def l1_subframe(words24, d29=0, d30=0):
    """Ten 24-bit source words (ints, d1 the highest bit) -> the 300 transmitted bits: D1..D24 = d ^ D30*, D25..D30 from the table,
    D29* / D30* carried from word to word starting at d29, d30 (the last two bits of the subframe before; out[-2:] continues the chain).
    A subframe whose first word starts with the preamble 0x8B goes out with the upright preamble when d30 is 0, inverted otherwise."""
    assert len(words24) == 10
    out = np.zeros(300, np.uint8)
    for i, w in enumerate(words24):
        d = [(int(w) >> (23 - k)) & 1 for k in range(24)]
        tx = [b ^ d30 for b in d]
        for star, idx in _L1_EQ:
            p = d29 if star == 29 else d30
            for k in idx:
                p ^= d[k - 1]
            tx.append(p)
        out[30 * i:30 * i + 30] = tx
        d29, d30 = tx[28], tx[29]
    return out


def crc24q_bits(bits):
    """CRC-24Q (polynomial 0x1864CFB, zero start) over a bit sequence, first bit highest"""
    crc = 0
    for b in bits:
        crc ^= int(b) << 23
        crc = ((crc << 1) ^ (0x1864CFB if crc & 0x800000 else 0)) & 0xFFFFFF
    return crc


def conv_encode_e1b(bits120):
    """K = 7, rate 1/2: per input bit the parities of the shift register (newest bit lowest) under G1 = 0x4f and G2 = 0x6d, G2 inverted
    -> 240 symbols"""
    sr, out = 0, []
    for b in bits120:
        sr = ((sr << 1) | int(b)) & 0x7F
        out.append(bin(sr & 0x4F).count("1") & 1)
        out.append((bin(sr & 0x6D).count("1") & 1) ^ 1)
    return np.array(out, np.uint8)


def e1b_page(word128_bits, alert=0, inverted=0, reserved=None, reserved2=None):
    """One nominal I/NAV page (Galileo OS SIS ICD 4.3.2.3): 128 word bits (the first 6 are the word type) -> 500 symbols, the even part
    then the odd part.  Even: even/odd 0, page type (= alert), word bits 0..111, 6 tail zeros.  Odd: even/odd 1, page type, word bits
    112..127, 64 bits of reserved 1 / SAR / spare (`reserved`, default zeros), CRC-24Q over the 114 + 82 bits before it, 8 bits of
    reserved 2, 6 tail zeros.  Each part: convolutional code, 30 x 8 block interleave (written by columns of 30), the 10-symbol
    preamble in front.  inverted: every symbol complemented."""
    w = np.asarray(word128_bits, np.uint8).reshape(-1)
    assert w.size == 128 and w.max(initial=0) <= 1
    res = np.zeros(64, np.uint8) if reserved is None else np.asarray(reserved, np.uint8).reshape(64)
    res2 = np.zeros(8, np.uint8) if reserved2 is None else np.asarray(reserved2, np.uint8).reshape(8)
    even = np.concatenate(([0, alert & 1], w[:112])).astype(np.uint8)
    odd = np.concatenate(([1, alert & 1], w[112:], res)).astype(np.uint8)
    crc = crc24q_bits(np.concatenate((even, odd)))
    crc_bits = np.array([(crc >> (23 - k)) & 1 for k in range(24)], np.uint8)
    parts = [np.concatenate((even, np.zeros(6, np.uint8))), np.concatenate((odd, crc_bits, res2, np.zeros(6, np.uint8)))]
    out = []
    for p in parts:
        assert p.size == 120
        enc = conv_encode_e1b(p)
        tx = enc.reshape(30, 8).T.reshape(-1)           # tx[c * 30 + r] = enc[r * 8 + c]
        out += [E1B_PREAMBLE, tx]
    out = np.concatenate(out).astype(np.uint8)
    return out ^ 1 if inverted else out
