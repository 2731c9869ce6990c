"""A plain Python / numpy model of nav frame sync (plain helper, imported like tests/fixtures.py; the product never imports it): the
`holding` loop of CHANNEL::Tracking(), ParityCheck, L1_parity and E1B_subframe written the way the reference writes them -- a buffer
of 0 / 1 values that is judged at its head and shifted, the parity equations on indexed bits with the in-place correction, the
Viterbi butterflies on a 64-entry metric array with a decision word per step, the chainback through `endstate` into a byte array,
checkcrc_e1b on the 25 right-aligned bytes through a CRC-24Q table.  It shares no code with flydog_sdr_gps_amd/csrc/kg_nav.h, which
works on packed words.  tests/golden/nav_ref.npz (the reference's own output) is what holds THIS model."""
import numpy as np

from flydog_sdr_gps_amd.nav import frame_dtype

L1, E1B = 0, 1
ERR_SLIP, ERR_CRC, ERR_ALERT, ERR_OOS, ERR_PAGE, ERR_PARITY = 1, 2, 3, 4, 5, 16
assert frame_dtype.itemsize == 64

L1_UP, L1_INV = [1, 0, 0, 0, 1, 0, 1, 1], [0, 1, 1, 1, 0, 1, 0, 0]
E1B_UP, E1B_INV = [0, 1, 0, 1, 1, 0, 0, 0, 0, 0], [1, 0, 1, 0, 0, 1, 1, 1, 1, 1]

_PAR = (
    (4, (1, 2, 3, 5, 6, 10, 11, 12, 13, 14, 17, 18, 20, 23)),
    (5, (2, 3, 4, 6, 7, 11, 12, 13, 14, 15, 18, 19, 21, 24)),
    (4, (1, 3, 4, 5, 7, 8, 12, 13, 14, 15, 16, 19, 20, 22)),
    (5, (2, 4, 5, 6, 8, 9, 13, 14, 15, 16, 17, 20, 21, 23)),
    (5, (1, 3, 5, 6, 7, 9, 10, 14, 15, 16, 17, 18, 21, 22, 24)),
    (4, (3, 5, 6, 8, 9, 10, 11, 13, 15, 19, 22, 23, 24)),
)


def l1_parity(p, buf, at):
    """L1_parity(p, buf + at, p[4], p[5]): corrects buf[at .. at + 24) in place, leaves the new parity in p -> differs"""
    d29, d30 = p[4], p[5]
    for i in range(24):
        buf[at + i] ^= d30
    new = []
    for which, idx in _PAR:
        v = d29 if which == 4 else d30
        for k in idx:
            v ^= buf[at + k - 1]
        new.append(v)
    p[:] = new
    return buf[at + 24:at + 30] != new


def _parity(x):
    return bin(x).count("1") & 1


BRANCH = [[255 if _parity((2 * s) & poly) else 0 for s in range(32)] for poly in (0x4F, 0x6D)]


def viterbi27(syms):
    """init_viterbi27_port(.., 0); update_viterbi27_blk_port(.., syms, 120); chainback_viterbi27_port(.., data, 114, 0) -> data[15]"""
    M = 0xFFFFFFFF
    old = [63] * 64
    old[0] = 0
    decisions = []
    for t in range(120):
        sym0, sym1 = syms[2 * t], syms[2 * t + 1]
        new, d = [0] * 64, 0
        for i in range(32):
            metric = (BRANCH[0][i] ^ sym0) + (BRANCH[1][i] ^ sym1)
            m0 = (old[i] + metric) & M
            m1 = (old[i + 32] + (510 - metric)) & M
            diff = (m0 - m1) & M
            dec = 1 if 0 < diff < 0x80000000 else 0
            new[2 * i] = m1 if dec else m0
            d |= dec << (2 * i)
            m0 = (m0 - (metric + metric - 510)) & M
            m1 = (m1 + (metric + metric - 510)) & M
            diff = (m0 - m1) & M
            dec = 1 if 0 < diff < 0x80000000 else 0
            new[2 * i + 1] = m1 if dec else m0
            d |= dec << (2 * i + 1)
        decisions.append(d)
        old = new
    data = [0] * 15
    endstate = 0
    nbits = 114
    while nbits != 0:
        nbits -= 1
        k = (decisions[6 + nbits] >> (endstate >> 2)) & 1
        endstate = (endstate >> 1) | (k << 7)
        data[nbits >> 3] = endstate & 0xFF
    return data


def getbitu(buff, pos, n):
    v = 0
    for i in range(pos, pos + n):
        v = (v << 1) + ((buff[i // 8] >> (7 - i % 8)) & 1)
    return v


def _crc_table():
    t = []
    for b in range(256):
        c = b << 16
        for _ in range(8):
            c = ((c << 1) ^ (0x1864CFB if c & 0x800000 else 0)) & 0xFFFFFF
        t.append(c)
    return t


CRC24Q = _crc_table()


def crc24q(buff):
    crc = 0
    for b in buff:
        crc = ((crc << 8) & 0xFFFFFF) ^ CRC24Q[(crc >> 16) ^ b]
    return crc


def checkcrc_e1b(d1, d2):
    bits = [(d1[i // 8] >> (7 - i % 8)) & 1 for i in range(114)] + [(d2[i // 8] >> (7 - i % 8)) & 1 for i in range(82)]
    bits = [0] * 4 + bits                               # bits2byte(.., 196, 25, right = 1, ..)
    bins = [int("".join(str(b) for b in bits[8 * i:8 * i + 8]), 2) for i in range(25)]
    return crc24q(bins) == getbitu(d2, 82, 24)


def e1b_subframe(fbits, polarity):
    """E1B_subframe on 500 symbols (0 / 1), polarity +1 / -1 -> (id, err, dec_e1b1, dec_e1b2)"""
    bits = [polarity * (-1 if b else 1) for b in fbits]
    dec = []
    for start in (10, 260):
        src = bits[start:start + 240]
        de = [src[c * 30 + r] for r in range(30) for c in range(8)]        # interleave(&bits[start], 30, 8, ..)
        enc = [(0 if v == 1 else 255) if i % 2 == 0 else (255 if v == 1 else 0) for i, v in enumerate(de)]
        dec.append(viterbi27(enc))
    d1, d2 = dec
    err, id = 0, 0
    if getbitu(d1, 0, 1):
        err = ERR_SLIP
    if not err and not checkcrc_e1b(d1, d2):
        id = getbitu(d1, 2, 6)
        err = ERR_CRC
    if not err and getbitu(d1, 1, 1) and getbitu(d2, 1, 1):
        err = ERR_ALERT
    if not err:
        buff = d1 + d2
        id = getbitu(buff, 2, 6)
        if id == 5:
            e1bhs = getbitu(buff, 2 + 69, 2)
            if e1bhs in (1, 3):
                err = ERR_OOS
            if getbitu(buff, 2 + 72, 1):
                err = ERR_OOS
    return id, err, d1, d2


class Channel:
    def __init__(self, mode):
        self.mode, self.sub = mode, 500 if mode == E1B else 300
        self.buf, self.base, self.pushed = [], 0, 0
        self.nav_ms = self.nav_prev = self.nav_glitch = 0

    def parity_check(self):
        """-> (record or None, nbits)"""
        buf = self.buf
        rec = np.zeros((), frame_dtype)
        rec["bit"] = self.base
        if self.mode == E1B:
            if buf[:10] == E1B_UP and buf[250:260] == E1B_UP:
                inverted = 0
            elif buf[:10] == E1B_INV and buf[250:260] == E1B_INV:
                inverted = 1
            else:
                return None, 1
            id, err, d1, d2 = e1b_subframe(buf[:500], -1 if inverted else 1)
            rec["err"], rec["id"], rec["inverted"] = err, id, inverted
            rec["data"][:30] = d1 + d2
            rec["consumed"] = 250 if err == ERR_SLIP else 500
            return rec, int(rec["consumed"])
        if buf[:8] == L1_UP:
            p = [0, 0, 0, 0, 0, 0]
        elif buf[:8] == L1_INV:
            p = [0, 0, 0, 0, 1, 1]
        else:
            return None, 1
        rec["inverted"] = p[5]
        for i in range(0, 300, 30):
            if l1_parity(p, buf, i):
                rec["err"], rec["id"], rec["consumed"] = ERR_PARITY, i // 30, i + 30
                return rec, i + 30
        rec["id"] = (buf[49] << 2) | (buf[50] << 1) | buf[51]
        rec["data"][:38] = np.packbits(np.array(buf[:300] + [0] * 4, np.uint8))
        rec["consumed"] = 300
        return rec, 300

    def push(self, bits):
        """-> [records]"""
        new = [int(b) & 1 for b in bits]
        self.buf += new
        self.pushed += len(new)
        out = []
        while len(self.buf) >= self.sub:
            rec, nbits = self.parity_check()
            if rec is not None:
                out.append(rec)
            del self.buf[:nbits]
            self.base += nbits
        return out

    def nav_bits(self, inavs):
        """the nav-bit machine of GPS_Method on one Inav per epoch -> the bits it saves"""
        out = []
        for inav in inavs:
            inav = int(inav)
            save = self.mode == E1B
            if not save:
                if inav != self.nav_prev:
                    self.nav_prev = inav
                    if self.nav_ms != 0:
                        self.nav_glitch = (self.nav_glitch + 1) & 0xFFFF
                    self.nav_ms = 1
                elif self.nav_ms != 19:
                    self.nav_ms += 1
                else:
                    save = True
            if save:
                self.nav_ms = 0
                out.append(inav)
        return out

    def state(self):
        return dict(holding=len(self.buf), bit0=self.base, held=np.array(self.buf, np.uint8), pushed=self.pushed,
                    nav_ms=self.nav_ms, nav_prev=self.nav_prev, nav_glitch=self.nav_glitch)


def frames(recs):
    return np.concatenate([np.asarray(r, frame_dtype).reshape(1) for r in recs]) if len(recs) else np.zeros(0, frame_dtype)


def run(mode, bits, cuts=None):
    """one stream through a fresh channel, in one push or in pushes of the sizes `cuts` (cycled) -> (frames, channel)"""
    c = Channel(mode)
    bits = list(np.asarray(bits).reshape(-1))
    recs, at, k = [], 0, 0
    if not cuts:
        recs = c.push(bits)
    else:
        while at < len(bits):
            n = cuts[k % len(cuts)]
            recs += c.push(bits[at:at + n])
            at += n
            k += 1
    return frames(recs), c
