"""Every entry point of include/kiwigpu.h that takes a pointer to device memory (`... *d_name`) is run with the host ahead of the
device by a case of tests/test_stream_order_gpu.py, or stands in the exemption table with its reason and the test that holds it to
stream order already.  An entry point added later with neither fails here."""
import importlib
import os
import re

from tests.test_containment_coverage_cpu import reachable_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULE = "test_stream_order_gpu"

# entry point -> (test function of tests/test_stream_order_gpu.py, how its source names the call)
REGISTRY = {
    "kg_wf_packets_dev": ("test_ring_wrap", "wf_packets_dev("),
    "kg_adpcm_encode_dev": ("test_cached_list_adpcm", "encode_dev("),
    "kg_post_process_dev": ("test_cached_list_post", "P.process_dev("),
    "kg_wf_frames_dev": ("test_waterfall_frame_tables", "frames_dev("),
    "kg_wf_frames_at_dev": ("test_waterfall_frame_tables", "frame_off="),
    "kg_wf_nb_frames_dev": ("test_waterfall_frame_tables", "nb_frames("),
    "kg_acq_sample_bits_dev": ("test_acq_pair_table_reuse", "s.sample("),
    "kg_acq_sample_iq16_dev": ("test_acq_samplers", "s.sample_iq16("),
    "kg_acq_sample_iq16_batch_dev": ("test_acq_samplers", "sample_iq16_batch("),
    "kg_fir_process_dev": ("test_fir", ".process_dev("),
    "kg_fir_process_each_dev": ("test_fir", "kg_fir_process_each_dev("),
    "kg_fir_process_taps_dev": ("test_fir", "kg_fir_process_taps_dev("),
    "kg_fir_refilter_dev": ("test_fir", "kg_fir_refilter_dev("),
    "kg_fir_process_spec_dev": ("test_fir", "process_spec_dev("),
    "kg_snd_spec_rows_dev": ("test_fir", "spec_rows_dev("),
    "kg_dpump_unpack_rows_dev": ("test_unpack_and_payloads", "unpack_rows_dev("),
    "kg_snd_iq_payload_dev": ("test_unpack_and_payloads", "kg_snd_iq_payload_dev("),
    "kg_snd_payload_dev": ("test_unpack_and_payloads", "kg_snd_payload_dev("),
    "kg_nb_process_dev": ("test_noise_blanker", "nb.process_dev("),
    "kg_aper_update_dev": ("test_aperture", "update_dev("),
    "kg_ddc_wf_push_dev": ("test_wf_ddc_inline", "d.push_dev("),                 # the in-line mode; deferred: MODES below
    "kg_ddc_wf_capture_dev": ("test_wf_ddc_inline", "capture_dev("),
    "kg_ddc_wf_step_dev": ("test_wf_ddc_inline", "kg_ddc_wf_step_dev("),
    "kg_rxddc_push_dev": ("test_rx_ddc", "d.push_dev("),
    "kg_post_nr_process_dev": ("test_post_nr", "nr_process_dev("),
    "kg_post_nrs_process_dev": ("test_post_nrs", "nrs_process_dev("),
    "kg_post_nbw_process_dev": ("test_post_nbw", "nbw_process_dev("),
    "kg_post_cfir_process_dev": ("test_post_cfir_and_squelch", "kg_post_cfir_process_dev("),
    "kg_post_squelch_perform_dev": ("test_post_cfir_and_squelch", "kg_post_squelch_perform_dev("),
    "kg_trk_process_bits_dev": ("test_tracker", "t.process_dev("),
    "kg_nav_push_bits_dev": ("test_nav_sync", "ns.push_dev("),
    "kg_nav_push_epochs_dev": ("test_nav_sync", "push_epochs_dev("),
    "kg_eph_push_frames_dev": ("test_ephemerides", "push_frames_dev("),
    "kg_eph_sv_dev": ("test_ephemerides", "sv_dev("),
    "kg_fftext_process_dev": ("test_fft_extension", "fx.process_dev("),
    "kg_iqd_process_dev": ("test_iq_display", "q.process_dev("),
}

# entry point -> (reason, test module, test function that holds it to stream order, or to the reference where order cannot matter)
EXEMPT = {
    "kg_pos_solve_dev": ("held to stream order by its own test: three solves with a reset and a mode change enqueued between them, one wait",
                         "test_pos_gpu", "test_reset_and_mode_in_stream_order"),
    "kg_rxbank_step": ("a bank plans, enqueues and commits a step on five streams of its own with its tables in an arena, not on one context's "
                       "ring: its back-to-back steps are held to the stepwise ones by the bank's tests", "test_receivers_gpu",
                       "test_adc_ring_refilled_without_host_synchronisation"),
    "kg_math_dev": ("a probe of the device's libm: no object, no table, no state", "test_libm_gpu", None),
    "kg_math_atan2f_dev": ("a probe of the device's libm: no object, no table, no state", "test_sam_libm_gpu", None),
    "kg_iqd_math_dev": ("a probe of the device's hypotf / fmodf: no object, no table, no state", "test_iqd_gpu", None),
    "kg_dpump_unpack_dev": ("synchronous by contract (it drains the stream before it returns); its enqueue-only twin kg_dpump_unpack_rows_dev has the "
                            "case", "test_snd_gpu", "test_unpack_bit_exact"),
}

# a mode of a registered entry point that the case does not run: (entry point, mode) -> (reason, test module, test function)
MODES = {
    ("kg_ddc_wf_push_dev", "deferred"): ("the deferred output stage runs on a stream of the object; twelve pushes with no wait are held to the oracle",
                                         "test_ddc_gpu", "test_deferred_output_stage_pipelines_pushes_bit_exact"),
}


def device_entry_points():
    with open(os.path.join(ROOT, "include", "kiwigpu.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    protos = re.findall(r"\b(kg_\w+)\s*\(([^;{}()]*)\)\s*;", text)
    assert len(protos) > 150, "the header did not parse: %d prototypes" % len(protos)
    return [name for name, args in protos if re.search(r"(?<!\*)\*\s*d_\w+", args)]       # `type *d_x`; not `type **d_x`, which hands a pointer out


def test_every_device_entry_point_runs_deep_or_is_exempt():
    names = device_entry_points()
    assert len(names) == len(set(names)) and {"kg_wf_packets_dev", "kg_iqd_process_dev", "kg_trk_process_bits_dev", "kg_rxbank_step"} <= set(names)
    missing = [n for n in names if n not in REGISTRY and n not in EXEMPT]
    assert not missing, "no stream-order case for %s: add one to tests/test_stream_order_gpu.py (tests/stream_order.py) and list it here" % missing
    stale = [n for n in list(REGISTRY) + list(EXEMPT) + [m[0] for m in MODES] if n not in names]
    assert not stale, "listed, but no longer a device entry point of the header: %s" % stale
    assert not set(REGISTRY) & set(EXEMPT)


def test_the_registered_cases_exist_and_call_their_entry_point():
    m = importlib.import_module("tests." + MODULE)
    for name, (fn, how) in REGISTRY.items():
        assert callable(getattr(m, fn, None)), (name, fn)
        assert how in reachable_source(m, fn), (name, "is not called in tests/%s.py::%s" % (MODULE, fn))


def test_the_exemptions_name_a_reason_and_a_test_that_exists():
    for key, (reason, mod, fn) in list(EXEMPT.items()) + list(MODES.items()):
        assert reason.strip(), key
        m = importlib.import_module("tests." + mod)
        assert fn is None or callable(getattr(m, fn, None)), (key, mod, fn)


def test_the_waterfall_case_knows_the_cache_ways():
    """tests/test_stream_order_gpu.py sizes its batches by WF_TABLE_WAYS of kg_wf.hip"""
    m = importlib.import_module("tests." + MODULE)
    with open(os.path.join(ROOT, "flydog_sdr_gps_amd", "csrc", "kg_wf.hip")) as f:
        ways = int(re.search(r"#define\s+WF_TABLE_WAYS\s+(\d+)", f.read()).group(1))
    assert m.WF_WAYS == ways
