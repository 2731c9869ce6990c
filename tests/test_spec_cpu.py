"""kg_spec.h, the audio spectrum display of c2s_sound() (specAF_FFT, rx/rx_sound.cpp:175-220) as kg_snd's kernels and the receiver
bank run it, compiled for the host with g++ -O2 -ffp-contract=off (the reference's flags) in the driver tools/spec_host_driver.cpp,
against the three pins of tests/golden/spec_ref.npz (made by tools/make_ref_spec_golden.py from the reference's own statements):
every byte of every row at both scales, the 125 ms limiter call by call, and the emission sequence block by block.  Then the
conditions the golden file must meet so that the parity tests cannot pass vacuously, kg_snd_spec_due through the C ABI, and the
prototypes."""
import os
import re

import numpy as np
import pytest

from . import spec_common as sc

ROOT = sc.ROOT
SPEC_SYMBOLS = {
    "kg_snd_spec_rows_dev": ("int kg_snd_spec_rows_dev(kg_ctx *ctx, const void *d_spec, size_t spec_stride, int nrows, const int32_t *inst, void *d_rows,", 7),
    "kg_snd_spec_due": ("int kg_snd_spec_due(uint32_t *last_ms, uint32_t now_ms);", 2),
    "kg_fir_process_spec_dev": ("int kg_fir_process_spec_dev(kg_fir *fir, const int32_t *chans, int nch, const void *d_in, size_t in_stride,", 14),
    "kg_rxbank_set_spec": ("int kg_rxbank_set_spec(kg_rxbank *bank, int rx, int n);", 3),
    "kg_rxbank_null_fir": ("kg_fir *kg_rxbank_null_fir(kg_rxbank *bank);", 1),
    "kg_rxbank_spec_max": ("int kg_rxbank_spec_max(kg_rxbank *bank);", 1),
    "kg_rxbank_spec_map": ("int kg_rxbank_spec_map(kg_rxbank *bank, int32_t *rx_of_row, int32_t *inst_of_row, int32_t *blk_of_row);", 4),
    "kg_rxbank_spec_rows": ("int kg_rxbank_spec_rows(kg_rxbank *bank, void **d_rows, size_t *row_stride);", 3),
}


@pytest.fixture(scope="module")
def golden():
    return sc.load()


@pytest.fixture(scope="module")
def pool():
    return sc.pool()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return sc.build_driver(tmp_path_factory.mktemp("spec"))


def test_pool_rebuilds(golden, pool):
    """the seeded spectra are the ones the reference binary was fed, and none holds a NaN (outside the row's contract)"""
    names, spec = pool
    assert names == [str(n) for n in golden["pool_names"]]
    assert sc.digest(spec.tobytes()) == bytes(golden["pool_sha"])
    assert not np.isnan(spec.real).any() and not np.isnan(spec.imag).any()
    assert sc.digest(sc.emit_blocks(int(golden["emit_nblocks"])).tobytes()) == bytes(golden["emit_blocks_sha"])


def test_rows_bit_exact(golden, pool, driver, tmp_path):
    """Pin 1: the host model equals the reference's rows byte for byte, both scales"""
    names, spec = pool
    got = sc.host_rows(driver, spec, tmp_path)
    want = golden["rows"]
    assert got.shape == want.shape == (len(names), 2, sc.W)
    for i, n in enumerate(names):
        for inst in (sc.PASSBAND, sc.CHAN_NULL):
            bad = np.flatnonzero(got[i, inst] != want[i, inst])
            assert bad.size == 0, (n, inst, "first differing byte", int(bad[0]), int(got[i, inst, bad[0]]), int(want[i, inst, bad[0]]))


def test_golden_file_meets_its_conditions(golden, pool):
    """conditions, not measurements: without them the parity tests could pass on a file that never leaves the easy path"""
    names, spec = pool
    rows = golden["rows"]
    ix = {n: i for i, n in enumerate(names)}
    assert len(names) * 2 >= 24
    assert rows.min() == 55 and rows.max() == 255                       # floor (-200 -> -201) and ceiling (0 -> -1)
    z = ix["zeros_signs_denormals"]
    unwrapped = lambda i, inst: rows[i, inst][np.arange(sc.W) ^ 512]    # row byte of bin b
    for inst in (0, 1):
        u = unwrapped(z, inst)
        assert (u[:256] == 55).all() and (u[768:] == 55).all()          # a zero bin (and -0.0): -300 -> -200 -> 55
        assert (u[512:640] == 55).all()                                 # denormals: the power underflows
    # re * re only: +-inf, overflowing powers -> 255; re = 0 beside a large (or infinite) im -> 55
    o = ix["inf_overflow_zero_re"]
    for inst in (0, 1):
        u = unwrapped(o, inst)
        assert (u[:192] == 255).all() and (u[256:512] == 55).all()
    # the sign of re does not matter: the pool's signs are random, the bytes of |re| equal (checked on the model in the GPU test too)
    # the half-swap: byte of bin b sits at b ^ 512 -- the edge rows are monotone in b before the swap
    e = unwrapped(ix["edge_pb_0"], 0).astype(int)
    assert (np.diff(e[:1000]) >= 0).all() and e[0] < e[999]
    # the edge set reaches both sides of the (int) truncation at every k from -200 to -1 (just below k the byte is one less than at
    # and above it; at k = 0 the clamp takes both sides to 255), and the nine values of a k span no more than one count
    for inst, n0 in ((0, "edge_pb_"), (1, "edge_null_")):
        u = np.concatenate([unwrapped(ix[n0 + "0"], inst), unwrapped(ix[n0 + "1"], inst)])[:201 * 9].reshape(201, 9).astype(int)
        assert (u.max(axis=1) - u.min(axis=1) <= 1).all()
        assert (u[:200, 0] == np.arange(55, 255)).all() and (u[:200, 8] == np.arange(56, 256)).all() and (u[200] == 255).all()
    # the two scales differ by 10 log10(1e6 / 0.0004) = 93.98 dB
    lu = ix["loguniform_0"]
    both = (rows[lu, 0] < 255) & (rows[lu, 1] > 55)
    d = rows[lu, 0][both].astype(int) - rows[lu, 1][both].astype(int)
    assert both.sum() > 100 and set(np.unique(d)) <= {93, 94, 95}
    assert os.path.getsize(os.path.join(sc.GOLD, "spec_ref.npz")) <= 300000


def test_limiter_equals_reference(golden, driver, tmp_path):
    """Pin 2: kg_spec::due call by call; and kg_snd_spec_due through the C ABI"""
    from flydog_sdr_gps_amd import snd
    scripts = sc.limiter_scripts()
    assert sorted(scripts) == [str(n) for n in golden["limiter_names"]]
    for k, clocks in scripts.items():
        assert np.array_equal(np.array(clocks, np.uint32), golden["limiter_%s_clock" % k]), k
        fired, last = sc.host_limiter(driver, clocks, tmp_path)
        assert np.array_equal(fired, golden["limiter_%s_fired" % k]), (k, fired, golden["limiter_%s_fired" % k])
        assert np.array_equal(last, golden["limiter_%s_last" % k]), k
        l = 0
        for i, c in enumerate(clocks):
            f, l = snd.spec_due(l, c)
            assert int(f) == int(fired[i]) and l == int(last[i]), (k, i)
    g = golden
    assert g["limiter_first_at_125_fired"][0] == 0 and g["limiter_first_at_125_fired"][1] == 1      # fires only when now > 125
    assert g["limiter_first_below_fired"][:5].sum() == 0
    assert g["limiter_first_above_fired"][0] == 1 and g["limiter_first_above_last"][0] == 126     # last = now the first time ...
    assert g["limiter_first_above_last"][g["limiter_first_above_fired"] == 1][1] == 251           # ... += 125 from then on
    for k in ("cadence_42_67", "cadence_25_28"):                                                      # about eight a second
        span = (int(g["limiter_%s_clock" % k][-1]) - int(g["limiter_%s_clock" % k][0])) / 1000.0
        assert abs(g["limiter_%s_fired" % k].sum() / span - 8.0) < 0.8, k
    # a long gap: += 125 catches up -- every call fires until last_ms is within 125 ms again; it never jumps to now
    f, l, c = g["limiter_long_gap_fired"], g["limiter_long_gap_last"], g["limiter_long_gap_clock"]
    assert f[12:12 + 30].all() and (np.diff(l[12:12 + 30].astype(np.int64)) == 125).all() and int(l[12]) < int(c[12]) - 3000


def test_emission_equals_reference(golden, driver, tmp_path):
    """Pin 3: the bank's emission rule (kg_spec::emit_block / emit_clear / cmd_on, the functions kg_rxbank.hip calls) on the golden
    scripts: per block the same rows in the same order -- instance, scale, which fill, every byte"""
    scripts = sc.emit_scripts()
    assert sorted(scripts) == [str(n) for n in golden["emit_names"]]
    blocks = sc.emit_blocks(int(golden["emit_nblocks"]))
    for k, lines in scripts.items():
        assert lines == [str(l) for l in golden["emit_%s_script" % k]], k
        got = sc.host_emit(driver, lines, blocks, tmp_path)
        want = sc.emit_golden(golden, k)
        assert len(got) == len(want), k
        for b, (gr, wr) in enumerate(zip(got, want)):
            assert [r[:3] for r in gr] == [r[:3] for r in wr], (k, "block", b, [r[:3] for r in gr], [r[:3] for r in wr])
            for r, w in zip(gr, wr):
                assert sc.digest(r[3].tobytes()) == w[3], (k, "block", b, r[:3])


def test_emission_golden_meets_its_conditions(golden):
    seq = lambda k: ["".join("PN"[r[0]] for r in b) for b in sc.emit_golden(golden, k)]
    w = seq("walk_spec_on")
    # USB x3, SAM(0) x3, SAM(null LSB) x4: the first block in channel null still gives a passband row, then its own; later only N
    assert w[:10] == ["P"] * 6 + ["PN", "N", "N", "N"]
    assert w[10:13] == ["P"] * 3                                          # the n == 5 re-send with mparam 0
    assert w[13:17] == ["PN", "N", "N", "N"] and w[17:20] == ["P"] * 3 and w[20:] == ["PN", "N", "N", "N"]
    assert all(s == "" for s in seq("walk_spec_off"))
    assert seq("on_off_on") == ["P"] * 3 + [""] * 3 + ["P"] * 3 + [""] * 6 + ["P"] * 2           # only 2 switches it on; 7 and -1 become 0
    assert seq("null_on_off_on") == [""] * 3 + ["N"] * 3 + [""] * 2 + ["N"] * 3                 # the second filter runs with the rows off
    # every row's scale flag is its instance: passband rows always x 1e6, channel-null rows x 0.0004
    for k in (str(n) for n in golden["emit_names"]):
        info = golden["emit_%s_info" % k]
        assert np.array_equal(info[:, 0], info[:, 1]), k
    # the fills are numbered across both filters: the channel-null filter fills at every block it is fed, rows on or not
    info = golden["emit_null_on_off_on_info"]
    assert info[:, 2].tolist() == [7, 9, 11, 17, 19, 21]


def test_spec_symbols_declared_bound_and_exported():
    from flydog_sdr_gps_amd import _lib
    header = open(os.path.join(ROOT, "include", "kiwigpu.h")).read()
    lib = _lib.load_library()
    for s, (proto, nargs) in SPEC_SYMBOLS.items():
        assert proto in header, s
        assert s in _lib.SYMBOLS and len(_lib.SYMBOLS[s][1]) == nargs, s
        assert hasattr(lib, s), s
    assert "#define KG_ABI_VERSION 4" in header or re.search(r"KG_ABI_VERSION\s*=?\s*4\b", header)
    h = {k: int(v) for k, v in re.findall(r"\bKG_(SPEC_[A-Z_]+)\s*=\s*(\d+)", header)}
    assert (h["SPEC_PASSBAND"], h["SPEC_CHAN_NULL"]) == (sc.PASSBAND, sc.CHAN_NULL)
    from flydog_sdr_gps_amd import snd
    assert (snd.SPEC_PASSBAND, snd.SPEC_CHAN_NULL) == (sc.PASSBAND, sc.CHAN_NULL)
    src = open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_spec.h")).read()
    for lit in ("WIDTH = 1024", "UPDATE_MS = 125", "PASSBAND = 0, CHAN_NULL = 1", "SPEC_SND_AF = 2, N_SND_SPEC = 3"):
        assert lit in src, lit
