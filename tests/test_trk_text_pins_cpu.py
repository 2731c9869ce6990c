"""The literals of the tracking channel, pinned by TEXT: parsed from the reference's Verilog, firmware and configuration and compared
with what the closed form (flydog_sdr_gps_amd/csrc/kg_trk.h), the literal model (tools/trk_model.cpp), the header and the binding
hold.  Nothing of the reference's text is kept here; the numbers are read where the reference tree is (REFERENCE, default
/root/reference)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE", "/root/reference")


def ref(rel):
    with open(os.path.join(REF, rel)) as f:
        return re.sub(r"//[^\n]*", "", f.read())


def our(rel):
    with open(os.path.join(ROOT, rel)) as f:
        return f.read()


def config(name):
    m = re.search(r"^\s*DEFp\s+%s\s+(0x[0-9a-fA-F]+|\d+)" % name, ref("kiwi.config"), re.M)
    assert m, name
    return int(m.group(1), 0)


CF, MODEL, HDR = our("flydog_sdr_gps_amd/csrc/kg_trk.h"), our("tools/trk_model.cpp"), our("include/kiwigpu.h")


def test_mixer_tables():
    v = ref("verilog/gps/demod.v")
    sin = re.search(r"lo_sin\s*=\s*4'b([01]{4})", v).group(1)
    cos = re.search(r"lo_cos\s*=\s*4'b([01]{4})", v).group(1)
    assert (int(sin, 2), int(cos, 2)) == (0xC, 0x6)
    assert re.search(r"LO_I\s*=\s*lo_sin\[lo_phase\[31:30\]\]", v) and re.search(r"LO_Q\s*=\s*lo_cos\[lo_phase\[31:30\]\]", v)
    assert "(0xCu >> top)" in CF and "(0x6u >> top)" in CF and "psi >> 30" in CF
    assert "lo_sin = 0x%X, lo_cos = 0x%X" % (int(sin, 2), int(cos, 2)) in MODEL


def test_ca_generator_taps():
    v = ref("verilog/gps/cacode.v")
    g1 = re.search(r"g1\[10:1\]\s*<=\s*\{g1\[9:1\],\s*([^}]*)\}", v).group(1)
    g2 = re.search(r"g2\[10:1\]\s*<=\s*\{g2\[9:1\],\s*([^}]*)\}", v).group(1)
    t1 = sorted(int(x) for x in re.findall(r"g1\[(\d+)\]", g1))
    t2 = sorted(int(x) for x in re.findall(r"g2\[(\d+)\]", g2))
    assert t1 == [3, 10] and t2 == [2, 3, 6, 8, 9, 10]
    assert re.search(r"T0\s*=\s*init\[8:5\]", v) and re.search(r"T1\s*=\s*init\[4:1\]", v)
    assert re.search(r"g1\s*<=\s*10'b1111111111", v) and re.search(r"g2\s*<=\s*g2_init\s*\?\s*init\s*:\s*10'b1111111111", v)
    # the closed form's table builder: stage i at bit i - 1
    assert "f1 = (%s) & 1" % " ^ ".join("(g1 >> %d)" % (t - 1) for t in t1) in CF
    assert "f2 = (%s) & 1" % " ^ ".join("(g2 >> %d)" % (t - 1) for t in t2) in CF
    assert "t0 = (init >> 4) & 15, t1 = init & 15" in CF
    # the literal model names the stages as the Verilog does
    assert "n.g1[1] = %s;" % " ^ ".join("d.g1[%d]" % t for t in t1) in MODEL
    assert "n.g2[1] = %s;" % " ^ ".join("d.g2[%d]" % t for t in t2) in MODEL


def test_widths_and_lengths():
    from flydog_sdr_gps_amd import sats, trk
    integ, repl, nav, e1b_mode, chans = (config(n) for n in ("GPS_INTEG_BITS", "GPS_REPL_BITS", "MAX_NAV_BITS", "E1B_MODE", "GPS_MAX_CHANS"))
    assert (integ, repl, nav, e1b_mode, chans) == (20, 18, 128, 0x800, 12)
    g2_init = int(re.search(r"#define\s+G2_INIT\s+(0x[0-9a-fA-F]+)", ref("gps/gps.h")).group(1), 0)
    for lit in ("INTEG_BITS = %d" % integ, "REPL_BITS = %d" % repl, "MAX_NAV_BITS = %d" % nav, "E1B_MODE = 0x%x" % e1b_mode, "G2_INIT = 0x%x" % g2_init,
                "L1_CODELEN = %d" % config("L1_CODELEN"), "E1B_CODELEN = %d" % config("E1B_CODELEN")):
        assert lit in CF, lit
    for lit in ("GPS_INTEG_BITS = %d" % integ, "MAX_NAV_BITS = %d" % nav, "E1B_MODE = 0x%x" % e1b_mode, "L1_CODELEN = %d" % config("L1_CODELEN"),
                "E1B_CODELEN = %d" % config("E1B_CODELEN")):
        assert lit in MODEL, lit
    for lit in ("KG_TRK_MAX_CHANS = %d" % chans, "KG_TRK_E1B_MODE = 0x%x" % e1b_mode, "KG_TRK_G2_INIT = 0x%x" % g2_init,
                "KG_TRK_E1B_CODELEN = %d" % config("E1B_CODELEN")):
        assert lit in HDR, lit
    assert (trk.MAX_CHANS, trk.E1B_MODE, trk.G2_INIT, trk.MAX_NAV_BITS) == (chans, e1b_mode, g2_init, nav)
    assert (sats.L1_CODELEN, sats.E1B_CODELEN) == (config("L1_CODELEN"), config("E1B_CODELEN"))
    # the 18-bit replica word
    v = ref("verilog/gps/demod.v")
    assert re.search(r"GPS_REPL_BITS == 18\) begin\s*assign replica = \{~cg_phase\[31\], cg_phase\[30:26\], chips\[9:0\], chips\[11:10\]\};", v)
    # ser_iq's order, E1B(0) only
    assert re.search(r"ser_iq <= \{ip, qp, ie, qe, il, ql\};", v)
    assert re.search(r"^\s*DEMOD #\(\.E1B\(0\)\) demod", ref("verilog/gps/gps.v"), re.M)


def test_gps_chan_field_order():
    from flydog_sdr_gps_amd import trk
    asm = re.sub(r";[^\n]*", "", ref("e_cpu/kiwi.gps.asm"))
    body = re.search(r"STRUCT\s+GPS_CHAN(.*?)ENDS", asm, re.S).group(1)
    fields = re.findall(r"(u16|u32|u64)\s+(\w+)\s+([^\n]+)", body)
    nav = config("MAX_NAV_BITS")
    size = {"u16": 2, "u32": 4, "u64": 8}
    def count(text):
        """the element counts the STRUCT uses: a number, `MAX_NAV_BITS / 16`, `2 * 3`"""
        m = re.fullmatch(r"\s*(\d+|MAX_NAV_BITS)\s*(?:([*/])\s*(\d+))?\s*", text)
        assert m, text
        a = nav if m.group(1) == "MAX_NAV_BITS" else int(m.group(1))
        if m.group(2) is None:
            return a
        return a * int(m.group(3)) if m.group(2) == "*" else a // int(m.group(3))

    got = [(n, size[t] * count(c)) for t, n, c in fields]
    want = [("ch_NAV_MS", 2), ("ch_NAV_BITS", 2), ("ch_NAV_GLITCH", 2), ("ch_NAV_PREV", 2), ("ch_NAV_BUF", 16), ("ch_CG_FREQ", 8), ("ch_LO_FREQ", 8),
            ("ch_IQ", 24), ("ch_CG_GAIN", 4), ("ch_LO_GAIN", 4), ("ch_unlocked", 2), ("ch_E1B_mode", 2), ("ch_LO_polarity", 2)]
    assert got == want
    assert sum(s for _, s in got) == trk.CHAN_BYTES == 78 and "KG_TRK_CHAN_BYTES = 78" in HDR and "CHAN_BYTES = 78" in CF
    # the binding's record: the same offsets under channel.cpp's names
    off, at = {}, 0
    for n, s in got:
        off[n] = at
        at += s
    names = {"ch_NAV_MS": "nav_ms", "ch_NAV_BITS": "nav_bits", "ch_NAV_GLITCH": "nav_glitch", "ch_NAV_PREV": "nav_prev", "ch_NAV_BUF": "nav_buf",
             "ch_CG_FREQ": "ca_freq", "ch_LO_FREQ": "lo_freq", "ch_IQ": "iq", "ch_CG_GAIN": "ca_gain", "ch_LO_GAIN": "lo_gain",
             "ch_unlocked": "ca_unlocked", "ch_E1B_mode": "E1B_mode", "ch_LO_polarity": "LO_polarity"}
    for n, f in names.items():
        assert trk.chan_dtype.fields[f][1] == off[n], n
    # struct UPLOAD of gps/channel.cpp lists the same members in the same order
    up = re.search(r"struct UPLOAD \{(.*?)\};", ref("gps/channel.cpp"), re.S).group(1)
    assert re.findall(r"uint16_t\s+(\w+)", up) == list(names.values())


def test_mult20_operand_widths():
    v = ref("verilog/cpu.v")
    assert re.search(r"xa20 = \(op8 == op_mult20\)\? nos\[19:0\]", v) and re.search(r"xb20 = \(op8 == op_mult20\)\? tos\[19:0\]", v)
    assert re.search(r"ipcore_mult_20b_20b_40b mult20\(\.P\(prod40\), \.A\(xa20\), \.B\(xb20\)\)", v)
    assert re.search(r"op_mult20\s*:\s*nos <= \{\{24\{prod40\[39\]\}\}, prod40\[39:32\]\}", v)
    assert "(int64_t) sext20(a) * (int64_t) sext20(b)" in CF and "(v << 12) >> 12" in CF
    assert "sext20_32(nos & 0xFFFFF) * (int64_t) sext20_32(tos & 0xFFFFF)" in MODEL


def test_nav_and_loop_literals():
    asm = ref("e_cpu/kiwi.gps.asm")
    assert re.search(r"push\s+19\s*\n\s*sub", asm)                       # 20 epochs per C/A bit
    assert "c.fw.nav_ms != 19" in CF and "ms - 19 == 0" in MODEL
    # the gains CHANNEL::SetGainAdjLO / CG send
    c = ref("gps/channel.cpp")
    assert re.search(r"int lo_ki = 20;\s*int lo_kp = 27;", c) and re.search(r"int ca_ki = 20-9;\s*int ca_kp = 27-4;", c)
    assert re.search(r"#define E1B_LO_GAIN_ADJ -3", c)
    from flydog_sdr_gps_amd import trk
    assert trk.gains(False) == ((20, 7), (11, 12)) and trk.gains(True) == ((17, 7), (11, 12))
    # the pause counter is 16 bits, one for the bank
    g = ref("verilog/gps/gps.v")
    assert re.search(r"reg\s+\[15:0\] cg_cnt;", g) and re.search(r"assign \{cg_resume, cg_nxt\} = cg_cnt - 1'b1;", g)
