"""Generates the reference-derived data the CPU tests pin against, so that they run without the reference tree:

  ref_text_pins.json  the literal tables and constants of reference files, parsed from their text: the CIC structure of the
                      generated verilog/rx/cic_*.vh, the CICF taps of verilog/rx/fir_iq.sv, the Sats[] rows of gps/sats.cpp,
                      the de-emphasis tables of rx/rx_filter.h, COEF / lo_sin / lo_cos of gps/search.cpp, the window and
                      CIC-compensation constants of rx/rx_waterfall.cpp and rx/CuteSDR/fastfir.cpp (+ rx/rx_sound.h's
                      WINF_SND_* numbers), and the parameters of the down-converters' Verilog that the DDC oracle and the exact
                      model of tests/ddc_exact.py rest on (verilog/rx/iq_mixer.v, cic_prune_var.v, rx.v, waterfall_1cic.v,
                      fir_iq.sv, resolved through verilog/kiwi.gen.vh) -- as numbers and signal names, evaluated here
  cacode_ref.npz      the C/A chips of every non-E1B row of Sats[], as the reference's own gps/cacode.h produces them
                      (oracle/_ref/cacode_ref, built by oracle/build_ref.sh)

Numbers only: no text of the reference is stored.  Run where the reference tree is present and oracle/_ref/ has been built:
REFERENCE=<reference tree> python tools/make_ref_text_golden.py"""
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
REFERENCE = os.environ.get("REFERENCE", "")
NUM = r"[-+]?(?:\d+\.\d*|\.\d+|\d+)(?:[eE][-+]?\d+)?"


def text(rel):
    return open(os.path.join(REFERENCE, rel)).read()


def lines(rel, lo, hi):
    return "".join(text(rel).splitlines(True)[lo - 1:hi])


def strip_comments(t):
    return re.sub(r"//[^\n]*", "", t)


def cic_vh(rel):
    """Structural constants of a generated verilog/rx/cic_*.vh: [N, R, Bin, Bout, integrator widths, comb widths,
    comb input truncations, [out msb, out width, rounding bit]]."""
    txt = text(rel)
    n, r, bin_, bout = (int(v) for v in re.search(r"N=(\d+) R=(\d+) M=1 Bin=(\d+) Bout=(\d+)", txt).groups())
    integ = [int(w) for w in re.findall(r"cic_integrator #\(\.WIDTH\((\d+)\)\)", txt)]
    comb = [int(w) for w in re.findall(r"cic_comb #\(\.WIDTH\((\d+)\)\)", txt)]
    trunc = []
    for blk in re.findall(r"cic_comb #.*?\);", txt, flags=re.S):
        src_w = re.search(r"\.in_data\((\w+)\[(\d+) -:(\d+)\]\)", blk)
        decl = re.search(r"wire signed \[(\d+):0\] %s;" % src_w.group(1), txt)
        trunc.append(int(decl.group(1)) + 1 - int(src_w.group(3)))      # declared width - bits taken
    m = re.search(r"assign out = comb\d_data\[(\d+) -:(\d+)\] \+ comb\d_data\[(\d+)\];", txt)
    return [n, r, bin_, bout, integ, comb, trunc, [int(v) for v in m.groups()]]


def fir_iq_sv():
    txt = text("verilog/rx/fir_iq.sv")
    branch = txt[txt.index("end else begin // N=5,R=3"):]
    default = [int(h, 16) for _, h in re.findall(r"assign taps\[\s*(\d+)\]\s*=\s*COEFF'\('sh([0-9a-fA-F]+)\);", branch)][:33]
    # the three `assign taps[..] = COEFF'('sh.....)` runs, in file order: RX_CFG == 3, == 14, default
    allt = [(int(i), int(h, 16)) for i, h in re.findall(r"assign taps\[\s*(\d+)\]\s*=\s*COEFF'\('sh([0-9a-f]{5})\)", txt)]
    sets, cur = [], []
    for i, v in allt:
        if i == 0 and cur:
            sets.append(cur)
            cur = []
        cur.append(v)
    sets.append(cur)
    return {"default_branch_taps": default, "tap_sets": sets}


def sats_rows():
    txt = text("gps/sats.cpp")
    body = txt[txt.index("SATELLITE Sats[] = {"):]
    body = body[:body.index("{-1}")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)          # the SBAS block is commented out
    body = re.sub(r"//[^\n]*", "", body)
    rows = re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\w+)\s*\}", body)
    lit = lambda v: int(v, 8) if len(v) > 1 and v[0] == "0" else int(v)      # noqa: E731 -- C literal: leading 0 = octal
    return [[int(p), lit(t1), lit(t2), kind] for p, t1, t2, kind in rows]


def rx_filter_h():
    txt = text("rx/rx_filter.h")
    tabs = {}
    for name in ("nfm_deemp_12000", "nfm_deemp_20250", "am_ssb_deemp_12000", "am_ssb_deemp_20250"):
        body = re.search(r"const float %s\[N_NFM_DEEMP\]\[N_DEEMP_TAPS\] = \{(.*?)\n\};" % name, txt, re.S).group(1)
        rows = re.findall(r"\{([^{}]*)\}", body)
        tabs[name] = [[float(v) for v in re.sub(r"//[^\n]*", "", r).replace("\n", " ").split(",") if v.strip()] for r in rows]
    return {"N_DEEMP_TAPS": int(re.search(r"#define N_DEEMP_TAPS (\d+)", txt).group(1)), "tables": tabs}


def search_cpp():
    txt = text("gps/search.cpp")
    body = re.search(r"static float COEF\[NTAPS\]\[2\][^=]*=\s*\{(.*?)\}\s*;", txt, re.S).group(1)
    lo = lines("gps/search.cpp", 380, 392)
    return {"FT": int(re.search(r"#define FT\s+(\d+)", txt).group(1)),
            "NTAPS": int(re.search(r"#define NTAPS\s+(\d+)", txt).group(1)),
            "COEF": [float(v) for v in re.findall(NUM, strip_comments(body))],
            "lo_sin": [int(v) for v in re.search(r"lo_sin\[\]\s*=\s*\{([^}]*)\}", lo).group(1).split(",")],
            "lo_cos": [int(v) for v in re.search(r"lo_cos\[\]\s*=\s*\{([^}]*)\}", lo).group(1).split(",")]}


def window_consts(t, prefix):
    out = {}
    for c in re.split(r"case %s" % prefix, t)[1:]:
        out[re.match(r"(\w+)", c).group(1)] = [float(v) for v in re.findall(r"(?<![\w.])(0\.\d+)(?![\w.])", c.split("break;")[0])]
    return out


def rx_waterfall_cpp():
    t = strip_comments(lines("rx/rx_waterfall.cpp", 128, 190))
    m = re.search(r"CIC_comp\[i\] = (%s) \+ cic_comp / (%s);" % (NUM, NUM), t)
    return {"adc_scale_decim_log2": float(re.search(r"adc_scale_decim = powf\(2, (-?\d+)\)", t).group(1)),
            "WINDOW_GAIN": float(re.search(r"#define WINDOW_GAIN\s+(%s)" % NUM, t).group(1)),
            "windows": window_consts(t, "WINF_WF_"),
            "cic_comp_p1": float(re.search(r"p1 = (%s)f" % NUM, t).group(1)),
            "cic_comp_p2": float(re.search(r"p2 = (%s)f" % NUM, t).group(1)),
            "cic_comp_offset": float(m.group(1)), "cic_comp_divisor": float(m.group(2)),
            "sincf_power": int(re.search(r"pow\(sincf, (-?\d+)\)", t).group(1))}


def fastfir_cpp():
    t = strip_comments(lines("rx/CuteSDR/fastfir.cpp", 61, 146))
    hdr = text("rx/rx_sound.h")
    names = ("BLACKMAN_NUTTALL", "BLACKMAN_HARRIS", "NUTTALL", "HANNING", "HAMMING")
    p = re.search(r"p1 = \(snd_rate == SND_RATE_3CH \? (%s)f : (%s)f\)" % (NUM, NUM), t)
    q = re.search(r"p2 = \(snd_rate == SND_RATE_3CH \? (%s)f\s*: (%s)f\s*\)" % (NUM, NUM), t)
    return {"WINF_SND": {n: int(re.search(r"#define WINF_SND_%s\s+(\d+)" % n, hdr).group(1)) for n in names},
            "windows": window_consts(t, "WINF_SND_"),
            "window_when_negative": re.search(r"window_func = WINF_SND_(\w+)", t).group(1),
            "cic_p1": [float(v) for v in p.groups()], "cic_p2": [float(v) for v in q.groups()]}


def _vparams(txt, env):
    """`localparam NAME = <integer expression>;` of a Verilog text, evaluated in order on top of env (names -> ints; clog2 as
    kiwi.gen.vh defines it: ceil(log2) above 1).  Only the values are kept."""
    out = dict(env)
    fns = {"clog2": lambda v: 1 if v <= 1 else (v - 1).bit_length()}
    for name, expr in re.findall(r"localparam\s+(\w+)\s*=\s*([^;?]+);", re.sub(r"//[^\n]*", "", txt)):
        if re.fullmatch(r"[\w\s+\-*()]+", expr):
            try:
                out[name] = int(eval(expr, {"__builtins__": {}}, dict(out, **fns)))      # noqa: S307 -- arithmetic on names only
            except (NameError, TypeError):
                pass
    return out


def _instances(txt, module, env):
    """Every `module #(.P(v), ...)` of a Verilog text: {P: value}, names resolved through env, strings kept."""
    res = []
    for body in re.findall(r"^\s*%s\s*#\((.*?)\)\s*$" % module, re.sub(r"//[^\n]*", "", txt), flags=re.M):
        inst = {}
        for k, v in re.findall(r"\.(\w+)\(\s*([^()]*(?:\([^()]*\))?[^()]*)\)", body):
            v = v.strip()
            inst[k] = v.strip('"') if v.startswith('"') else int(eval(v, {"__builtins__": {}}, dict(env)))      # noqa: S307
        res.append(inst)
    return res


def verilog_ddc():
    gen = text("verilog/kiwi.gen.vh")
    env = _vparams(gen, {})
    by_cfg = {}
    for name in ("RX1_DECIM", "RX2_DECIM"):                  # the RX_CFG ladders: configuration -> decimation
        ladder = re.search(r"localparam %s = ([^;]+);" % name, gen).group(1)
        by_cfg[name] = {cfg: env[sym] for cfg, sym in re.findall(r"\(RX_CFG == (\d+)\)\?\s*(\w+)", ladder)}
    # iq_mixer.v
    mix_txt = text("verilog/rx/iq_mixer.v")
    mixer = {"for_OUT_WIDTH": {}}
    for w in (env["RX1_BITS"], env["WF1_BITS"]):
        pm = _vparams(mix_txt, {"IN_WIDTH": env["ADC_BITS"], "OUT_WIDTH": w})
        mixer["for_OUT_WIDTH"][str(w)] = {k: pm[k] for k in ("ZFILL", "SIGN", "MANTISSA", "MANTISSA_W", "RND")}
    code = re.sub(r"//[^\n]*", "", mix_txt)
    m = re.search(r"assign out_i = \{ prod_i\[(\w+)\], prod_i\[(\w+) -:(\w+)\] \} \+ prod_i\[(\w+)\];", code)
    mixer["out_slice_names"] = list(m.groups())              # {sign bit, [msb -: width]} + [rounding bit]
    hi, = re.findall(r"wire signed \[(\d+):0\] dds_sin, dds_cos;", code)
    fill, = re.findall(r"assign cos = \{dds_cos, (\d+)'b0\};", code)
    fac, = re.findall(r"reg signed \[(\d+):0\] mx, my_i, my_q;", code)
    prod, = re.findall(r"reg signed \[(\d+):0\] prod_i, prod_q;", code)
    pinc, = re.findall(r"input wire signed \[(\d+):0\] phase_inc", code)
    mixer.update(dds_bits=int(hi) + 1, dds_zero_fill=int(fill), factor_bits=int(fac) + 1, product_bits=int(prod) + 1,
                 phase_bits=int(pinc) + 1, i_from=re.search(r"my_i <= (\w+);", code).group(1), q_from=re.search(r"my_q <= (\w+);", code).group(1))
    # waterfall_1cic.v and rx.v: what they instantiate
    wf_txt, rx_txt = text("verilog/rx/waterfall_1cic.v"), text("verilog/rx/rx.v")
    wenv = _vparams(wf_txt, dict(env, IN_WIDTH=env["ADC_BITS"]))
    wf_cic = _instances(wf_txt, "cic_prune_var", wenv)
    assert wf_cic[0] == wf_cic[1]                            # I and Q
    inst = {"waterfall_1cic_v": {"IQ_MIXER": _instances(wf_txt, "IQ_MIXER", wenv)[0], "cic_prune_var": wf_cic[0]}, "rx_v": {}}
    for cfg in sorted(by_cfg["RX1_DECIM"], key=int):
        renv = _vparams(rx_txt, dict(env, IN_WIDTH=env["ADC_BITS"], RX1_DECIM=by_cfg["RX1_DECIM"][cfg], RX2_DECIM=by_cfg["RX2_DECIM"][cfg]))
        cics = _instances(rx_txt, "cic_prune_var", renv)
        assert cics[0] == cics[1] and cics[2] == cics[3]
        inst["rx_v"][cfg] = {"IQ_MIXER": _instances(rx_txt, "IQ_MIXER", renv)[0], "rx1": cics[0], "rx2": cics[2],
                             "fir_iq": _instances(rx_txt, "fir_iq", renv)[0]}
    m = re.search(r"rx_dout = rd_i\? rx_cic_out_(\w)\[(\d+):0\] : \( rd_q\? rx_cic_out_(\w)\[(\d+):0\] : "
                  r"\{rx_cic_out_(\w)\[RXO_BITS-1 -:(\d+)\], rx_cic_out_(\w)\[RXO_BITS-1 -:(\d+)\]\} \)", rx_txt)
    g = m.groups()                                           # 16-bit words: low 16 of i, low 16 of q, {top 8 of .., top 8 of ..}
    inst["rx_v"]["words"] = [[g[0], int(g[1]) + 1], [g[2], int(g[3]) + 1], [g[4], int(g[5]), g[6], int(g[7])]]
    # cic_prune_var.v: the variable pre-shift of the instance the waterfall builds, and the R = 1 slice
    cp_txt = re.sub(r"//[^\n]*", "", text("verilog/rx/cic_prune_var.v"))
    w = wf_cic[0]
    cenv = _vparams(cp_txt, dict(env, IN_WIDTH=w["IN_WIDTH"], OUT_WIDTH=w["OUT_WIDTH"], STAGES=w["STAGES"], GROWTH=w["GROWTH"]))
    block = cp_txt[cp_txt.index("if (DECIMATION == %d)" % w["DECIMATION"]):]
    block = block[:block.index("endgenerate")]
    cases = []
    for d, rhs in re.findall(r"^\s*(\d+): in <= ([^;]+);", block, flags=re.M):
        sh = re.fullmatch(r"in_data << \((\w+) - (\w+)\)", rhs.strip())
        cases.append([int(d), cenv[sh.group(1)] - cenv[sh.group(2)] if sh else 0])
    s1 = re.search(r"if \(decim == 1\)\s*out_data <= in\[([\w\-]+) -:(\w+)\];", cp_txt)
    cnt = re.search(r"if \(sample_no == \(decim-(\d+)\)\)", cp_txt)
    prune = {"ACC_WIDTH": cenv["ACC_WIDTH"], "decim_shift": cases, "default_shift": 0 if re.search(r"default: in <= in_data;", block) else None,
             "r1_slice": [int(eval(s1.group(1), {"__builtins__": {}}, dict(cenv))), cenv[s1.group(2)]],      # noqa: S307 -- [msb, width]
             "strobe_when_sample_no_is_decim_minus": int(cnt.group(1)),
             "fixed_decimation_shift": 0 if re.search(r"if \(DECIMATION > 0\)\s*begin\s*always @\(posedge clock\)\s*in <= in_data;", cp_txt) else None}
    # fir_iq.sv: the decimate-by-2 flag
    fir_txt = re.sub(r"//[^\n]*", "", text("verilog/rx/fir_iq.sv"))
    fenv = _vparams(fir_txt, dict(env, WIDTH=env["RXO_BITS"]))
    init = re.findall(r"initial decim_by_2 = (\d);", fir_txt)
    run = fir_txt[fir_txt.index("STATE_COMPUTE_SUM && next_state == STATE_COPY_OUTPUT"):]
    run = run[:run.index("end")]
    emits = re.findall(r"out_strobe <= (~|!)?decim_by_2;", run)
    toggles = re.findall(r"decim_by_2 <= decim_by_2 \^ 1'b1;", run)
    nt = re.search(r"localparam NTAPS = \(RX_CFG == (\d+) \? (\d+) : (\d+)\);", fir_txt)
    fir = {"COEFF": fenv["COEFF"], "ACCW": fenv["ACCW"], "ACCOUT": fenv["ACCOUT"], "out_slice_names": list(re.search(
               r"out_data_i <= accI\[(\w+) -:(\w+)\];", run).groups()),
           "NTAPS": {nt.group(1): int(nt.group(2)), "other": int(nt.group(3))}}
    if len(init) == 1 and len(emits) == 1 and len(toggles) == 1:          # unambiguous: one initial value, one strobe, one toggle per input
        fir["decim_by_2_initial"] = int(init[0])
        fir["decim_by_2_value_that_emits"] = 0 if emits[0] else 1
    return {"params": {k: env[k] for k in ("ADC_BITS", "RX1_BITS", "RX2_BITS", "RXO_BITS", "RX1_STAGES", "RX2_STAGES", "WF1_BITS", "WFO_BITS",
                                          "WF1_STAGES", "WF_1CIC_MAXD", "RX1_STD_DECIM", "RX2_STD_DECIM", "RX1_WIDE_DECIM", "RX2_WIDE_DECIM")},
            "decim_by_RX_CFG": by_cfg, "iq_mixer_v": mixer, "instances": inst, "cic_prune_var_v": prune, "fir_iq_sv": fir}


def cacode_chips():
    from flydog_sdr_gps_amd import sats
    exe = os.path.join(ROOT, "oracle", "_ref", "cacode_ref")
    taps, chips = [], []
    for _, t1, t2, kind in sats.SATS:
        if kind == sats.E1B:
            continue
        s = subprocess.check_output([exe, str(t1), str(t2)]).decode().strip()
        taps.append((t1, t2))
        chips.append(np.frombuffer(s.encode(), np.uint8) - ord("0"))
    return np.array(taps, np.int32), np.packbits(np.stack(chips), axis=1)


def main():
    if not os.path.isfile(os.path.join(REFERENCE, "gps", "sats.cpp")):
        sys.exit("make_ref_text_golden.py: set REFERENCE to the reference tree")
    pins = {"_source": "tools/make_ref_text_golden.py: numbers parsed from the reference's text",
            "cic_vh": {f: cic_vh("verilog/rx/" + f) for f in ("cic_wf1.vh", "cic_rx1_12k.vh", "cic_rx2_12k.vh")},
            "fir_iq_sv": fir_iq_sv(), "sats_cpp": sats_rows(), "rx_filter_h": rx_filter_h(), "search_cpp": search_cpp(),
            "rx_waterfall_cpp": rx_waterfall_cpp(), "fastfir_cpp": fastfir_cpp(), "verilog_ddc": verilog_ddc()}
    with open(os.path.join(GOLD, "ref_text_pins.json"), "w") as f:
        json.dump(pins, f, indent=1)
        f.write("\n")
    taps, packed = cacode_chips()
    np.savez_compressed(os.path.join(GOLD, "cacode_ref.npz"), taps=taps, chips_packed=packed)
    print("wrote tests/golden/ref_text_pins.json, tests/golden/cacode_ref.npz (%d C/A rows)" % len(taps))


if __name__ == "__main__":
    main()
