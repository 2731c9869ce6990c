"""Generates tests/golden/nav_ref.npz from the REFERENCE ITSELF: the frame-sync part of CHANNEL::Tracking() (gps/channel.cpp: the
`holding` loop, ParityCheck, L1_parity) with E1B_subframe, checkcrc_e1b and KA9Q's Viterbi decoder behind it.

Runs on the CPU machine only, where the reference tree is present ($REFERENCE, default /root/reference); no test, smoke() or bench
reads the reference.  In the manner of tools/make_ref_sam_golden.py it cuts line ranges of the reference into a temporary directory
(deleted on exit), checks the text at both ends of every cut and the text of the statements the harness restates, compiles
tools/ref/ref_nav_main.cpp around them with gps/ka9q-fec/viterbi27_port.cpp linked where it lies, runs it on seeded streams (built
here with the encoders of flydog_sdr_gps_amd/nav.py) and keeps only data: the streams and the records the reference's code printed.
That the reference accepts the encoders' frames with err == 0 is the proof that the encoders are right; the conditions at the end
keep every later test from passing on an empty set.

    python tools/make_ref_nav_golden.py
"""
import os
import subprocess
import tempfile

import numpy as np

import ref_cut
from ref_cut import R, ROOT  # ref_cut puts the repository root on sys.path
from flydog_sdr_gps_amd import nav  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
CH, GAL, NAVC, RTK = "gps/channel.cpp", "gps/GNSS-SDRLIB/sdrnav_gal.cpp", "gps/GNSS-SDRLIB/sdrnav.cpp", "gps/GNSS-SDRLIB/rtkcmn.cpp"

# (file, macro, first, last, text of the first line, text of the last line)
CUTS = [
    ("gps/gps.h", "NAV_CUT_GPSERR", 187, 191, "#define GPS_ERR_SLIP    1", "#define GPS_ERR_PAGE    5"),
    (RTK, "NAV_CUT_CRCTAB", 271, 304, "static const unsigned int tbl_CRC24Q[]={", "};"),
    (RTK, "NAV_CUT_GETBITU", 598, 604, "extern unsigned int getbitu(", "}"),
    (RTK, "NAV_CUT_CRC24Q", 662, 671, "extern unsigned int crc24q(", "}"),
    (NAVC, "NAV_CUT_SDRNAV", 154, 190, "extern void bits2byte(", "}"),
    (GAL, "NAV_CUT_OFFSETS", 19, 20, "#define OFFSET1     2", "#define OFFSET2     122"),
    (GAL, "NAV_CUT_WORD5", 162, 174, "e5bhs          =getbitu(buff,OFFSET1+67, 2);", "}"),
    (GAL, "NAV_CUT_CHECKCRC", 293, 319, "extern int checkcrc_e1b(", "}"),
    (GAL, "NAV_CUT_E1B_SUBFRAME", 382, 514, "extern int E1B_subframe(sdrnav_t *nav, int *error)", "}"),
    (CH, "NAV_CUT_PREAMBLES", 120, 145, "#define L1_PRELEN 8", "const char E1BpreambleInverse [] = {1,0,1,0,0,1,1,1,1,1};"),
    (CH, "NAV_CUT_POLYS", 414, 416, "int polys[2] = { 0x4f, 0x6d };", "nav.fec = create_viterbi27_port(E1B_NBIT);"),
    (CH, "NAV_CUT_LOOP", 452, 506, "while (holding >= subframe_bits) {", "memmove(buf, buf+nbits, holding-=nbits);"),
    (CH, "NAV_CUT_PARITYCHECK", 731, 832, "int CHANNEL::ParityCheck(char *buf, int *nbits) {", "}"),
]
# what the harness restates: (file, line, text)
PINS = [
    ("gps/GNSS-SDRLIB/gnss_sdrlib.h", 136, "#define MAXBITS       3000"),
    (CH, 399, "holding=0;"), (CH, 404, "nsync = 0;"), (CH, 405, "total_bits = 0;"), (CH, 406, "expecting_preamble = 0;"),
    (CH, 407, "drop_seq = 0;"), (CH, 278, "subframe_bits = isE1B? E1B_TSYM_PW : 300;"), (CH, 445, "buf[holding++] = (word >> 16) & 1;"),
    (GAL, 334, "memcpy(buff,buff1,15); memcpy(&buff[15],buff2,15);"), (GAL, 336, "id=getbitu(buff,2,6); /* word type */"),
    (GAL, 346, "case  5: decode_word5(buff, nav, &err); break;"), (GAL, 357, "if (err && error) *error = err;"),
    (GAL, 152, "void decode_word5(const uint8_t *buff, sdrnav_t *nav, int *error)"),
    ("gps/ka9q-fec/viterbi27_port.cpp", 13, "typedef union { unsigned long w[2];} decision_t;"),
]


def build(tmp):
    ref_cut.cut(tmp, CUTS)
    ref_cut.pin(PINS)
    exe = os.path.join(tmp, "nav_ref")
    cmd = (["g++", "-O2", "-w", "-std=gnu++11", "-I" + os.path.join(R, "gps", "ka9q-fec"), "-I" + tmp] +
           ref_cut.cut_macros(CUTS) +
           ["-o", exe, os.path.join(ROOT, "tools", "ref", "ref_nav_main.cpp"), os.path.join(R, "gps", "ka9q-fec", "viterbi27_port.cpp")])
    subprocess.run(cmd, check=True)
    return exe


def run_ref(exe, mode, bits):
    script = "T %d\nP %s\n" % (mode, "".join("01"[int(b) & 1] for b in bits))
    p = subprocess.run([exe], input=script.encode(), stdout=subprocess.PIPE, check=True)
    recs, hold = [], None
    for line in p.stdout.decode().splitlines():
        f = line.split()
        if f[0] == "F":
            r = np.zeros((), nav.frame_dtype)
            r["bit"], r["err"], r["consumed"], r["inverted"], r["id"] = (int(v) for v in f[1:6])
            r["data"] = np.frombuffer(bytes.fromhex(f[6]), np.uint8)
            recs.append(r.reshape(1))
        elif f[0] == "H":
            hold = (int(f[1]), int(f[2]))
    return (np.concatenate(recs) if recs else np.zeros(0, nav.frame_dtype)), hold


# ---- the streams
rng = np.random.Generator(np.random.PCG64(0x4E41560001))


def rbits(n):
    return rng.integers(0, 2, n).astype(np.uint8)


def ca_frames(n, sub0=1, d29=0, d30=0):
    """n consecutive subframes with random payloads, ids sub0, sub0 + 1, ... (1..5), the parity chain carried through"""
    out = []
    for k in range(n):
        w = [int(v) for v in rng.integers(0, 1 << 24, 10)]
        w[0] = (0x8B << 16) | (w[0] & 0xFFFF)
        w[1] = (w[1] & ~(7 << 2)) | ((((sub0 + k - 1) % 5) + 1) << 2)
        f = nav.l1_subframe(w, d29, d30)
        while f[-2] or f[-1]:                                           # as the system does with word 10's last two data bits: D29 = D30 = 0
            w[9] = int(rng.integers(0, 1 << 24))
            f = nav.l1_subframe(w, d29, d30)
        d29, d30 = int(f[-2]), int(f[-1])
        out.append(f)
    return out


def word128(wtype, fill=None):
    w = rbits(128) if fill is None else np.full(128, fill, np.uint8)
    w[:6] = [(wtype >> (5 - k)) & 1 for k in range(6)]
    return w


def pages(types, **kw):
    return [nav.e1b_page(word128(t), reserved=rbits(64), reserved2=rbits(8), **kw) for t in types]


def flip(bits, at):
    bits = bits.copy()
    bits[list(at)] ^= 1
    return bits


def scenarios():
    S = []                                                              # (name, mode, bits, how many untouched frames of the encoders it holds at least)
    L1, E1B = nav.L1, nav.E1B
    S.append(("ca_upright", L1, np.concatenate(ca_frames(4) + [rbits(37)]), 4))
    S.append(("ca_inverted", L1, np.concatenate(ca_frames(4, sub0=3) + [rbits(55)]) ^ 1, 4))
    f = ca_frames(4, sub0=2)
    S.append(("ca_flip_between", L1, np.concatenate(f[:2] + [f[2] ^ 1, f[3] ^ 1, rbits(20)]), 4))
    S.append(("ca_leading_random", L1, np.concatenate([rbits(411)] + ca_frames(3, sub0=5) + [rbits(100)]), 3))
    for k in range(10):                                                 # one bit wrong in word k of the second subframe
        f = ca_frames(3, sub0=k)
        f[1] = flip(f[1], [30 * k + int(rng.integers(8 if k == 0 else 0, 30))])
        S.append(("ca_bit_error_w%d" % k, L1, np.concatenate([rbits(13)] + f + [rbits(290)]), 1))
    f = ca_frames(3)
    f[1] = flip(f[1], [3])
    S.append(("ca_preamble_error", L1, np.concatenate(f + [rbits(150)]), 2))
    for k in range(3):                                                  # hunting through random data: false preambles
        S.append(("ca_random_%d" % k, L1, np.concatenate([rbits(700 + 97 * k)] + ca_frames(2, sub0=k + 1) + [rbits(120)]), 0))
    # a false frame whose first five words hold, 150 bits before a true frame: its failure at a middle word swallows the true start
    fa, tr = ca_frames(1)[0], ca_frames(3, sub0=2)
    S.append(("ca_swallowed_start", L1, np.concatenate([rbits(5), fa[:150]] + tr + [rbits(60)]), 0))
    S.append(("ca_short", L1, np.concatenate([ca_frames(1)[0][:260]]), 0))
    S.append(("ca_back_to_back_preambles", L1, np.concatenate([np.tile(np.concatenate([nav.L1_PREAMBLE, rbits(22)]), 1)
                                                               for _ in range(40)]), 0))

    S.append(("e1b_upright", E1B, np.concatenate(pages([1, 2, 3, 4, 0]) + [rbits(77)]), 5))
    S.append(("e1b_inverted", E1B, np.concatenate([rbits(33)] + pages([2, 4, 6, 10, 1], inverted=1) + [rbits(40)]), 5))
    p = pages([1, 3, 6, 7])                                             # a start on an odd half, and half a page lost in mid-stream
    S.append(("e1b_odd_start", E1B, np.concatenate([p[0][250:], p[1], p[2][250:], p[3], rbits(300)]), 2))
    p = pages([2, 4, 0], inverted=1)
    S.append(("e1b_odd_start_inverted", E1B, np.concatenate([rbits(9), p[0][250:]] + p[1:] + [rbits(260)]), 2))
    p = pages([1, 2, 3, 4, 6])
    for k, pg in enumerate(p):                                          # 1..3 symbol errors in each half, outside the preambles
        for half in (0, 250):
            pg[half + 10 + rng.choice(240, 1 + (k + half // 250) % 3, replace=False)] ^= 1
    S.append(("e1b_symbol_errors", E1B, np.concatenate(p + [rbits(64)]), 5))
    p = pages([1, 2, 3, 4, 5, 6])
    for k in (0, 1, 2, 3, 4):                                           # a burst the decoder cannot mend, in the even or the odd half:
        idx = np.array([(k % 2) * 250 + 10 + c * 30 + r for r in range(8 + k, 20 + k) for c in range(8)])   # 96 consecutive coded symbols
        p[k][idx] ^= rbits(96) | (np.arange(96) % 2 == 0).astype(np.uint8)
    S.append(("e1b_bursts", E1B, np.concatenate(p), 1))
    S.append(("e1b_alert", E1B, np.concatenate(pages([1, 5], alert=1) + pages([2, 3]) + pages([4], alert=1, inverted=0) + [rbits(10)]), 2))
    w5 = []
    for hs, dvs in ((0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (2, 1)):    # decode_word5: e1bhs at word bits 69..70, e1bdvs at 72
        w = word128(5)
        w[69], w[70], w[72] = hs >> 1, hs & 1, dvs
        w5.append(nav.e1b_page(w, reserved=rbits(64)))
    S.append(("e1b_word5_health", E1B, np.concatenate(w5), 2))                  # the other four are OOS
    S.append(("e1b_high_types", E1B, np.concatenate(pages([17, 63, 11, 0]) + [rbits(130)]), 4))
    # a preamble pair forced inside a page: the stream starts 100 symbols into a page and symbols 20.. and 270.. are overwritten
    p = pages([1, 2, 3, 4])
    lead = p[0][100:].copy()
    lead[20:30] = nav.E1B_PREAMBLE
    lead[270:280] = nav.E1B_PREAMBLE
    S.append(("e1b_chance_pair_in_page", E1B, np.concatenate([lead] + p[1:] + [rbits(50)]), 2))
    p = pages([1, 2, 3, 4])
    p[1][250:] ^= 1                                                     # the second preamble in the other polarity: no match at that head
    S.append(("e1b_mixed_polarity_page", E1B, np.concatenate(p + [rbits(90)]), 3))
    S.append(("e1b_all_zero_all_one", E1B, np.concatenate([nav.e1b_page(word128(0, 0)), nav.e1b_page(word128(63, 1), reserved=np.ones(64, np.uint8),
                                                                                                  reserved2=np.ones(8, np.uint8)),
                                                           nav.e1b_page(word128(0, 0), inverted=1), rbits(20)]), 3))
    S.append(("e1b_short", E1B, pages([1])[0][:499], 0))
    return S


def main():
    out, names = {}, []
    tally = dict(ca_ok=0, ca_par_hi=0, ca_par=set(), e1b_ok=0, slip=0, crc=0, alert=0, oos=0, pol=set())
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name, mode, bits, nenc in scenarios():
            bits = np.asarray(bits, np.uint8) & 1
            fr, hold = run_ref(exe, mode, bits)
            names.append(name)
            out[name + "_mode"] = np.array([mode], np.int32)
            out[name + "_nbits"] = np.array([bits.size], np.int32)
            out[name + "_bits"] = np.packbits(bits)
            out[name + "_frames"] = fr.view(np.uint8).reshape(-1, 64)
            out[name + "_hold"] = np.array(hold, np.int64)
            ok = int((fr["err"] == 0).sum())
            assert ok >= nenc, (name, "the reference refused a frame of the encoders", ok, nenc)
            for r in fr:
                tally["pol"].add((mode, int(r["inverted"])))
                if mode == nav.L1:
                    tally["ca_ok"] += r["err"] == 0
                    if r["err"] == nav.ERR_PARITY:
                        tally["ca_par"].add(int(r["id"]))
                        tally["ca_par_hi"] += r["id"] > 0
                else:
                    tally["e1b_ok"] += r["err"] == 0
                    tally["slip"] += r["err"] == nav.ERR_SLIP
                    tally["crc"] += r["err"] == nav.ERR_CRC
                    tally["alert"] += r["err"] == nav.ERR_ALERT
                    tally["oos"] += r["err"] == nav.ERR_OOS
            print("nav_ref.npz: %-28s mode %d  %5d bits  %3d records (%d ok)  holding %d from bit %d" % (name, mode, bits.size, len(fr), ok, *hold))
    print({k: (sorted(v) if isinstance(v, set) else int(v)) for k, v in tally.items()})
    assert tally["ca_ok"] >= 20 and tally["ca_par_hi"] >= 5 and tally["e1b_ok"] >= 20, tally
    assert tally["slip"] >= 3 and tally["crc"] >= 5 and tally["alert"] >= 1 and tally["oos"] >= 2, tally
    assert tally["pol"] == {(0, 0), (0, 1), (1, 0), (1, 1)}, tally
    assert tally["ca_par"] >= set(range(10)), tally                     # a parity failure at every word index
    out["names"] = np.array(names)
    path = os.path.join(GOLD, "nav_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
