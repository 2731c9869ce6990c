"""Every entry point of include/kiwigpu.h that takes a pointer to caller device memory (`void *d_...` / `const void *d_...`) has a
containment case (tests/test_containment_*_gpu.py), or stands in the exemption list with its reason.  An entry point added later
without a case fails here."""
import importlib
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry point -> (test module, test function) that runs it on the guarded layouts
REGISTRY = {
    "kg_adpcm_encode_dev": ("test_containment_gpu", "test_adpcm_encode"),
    "kg_snd_payload_dev": ("test_containment_gpu", "test_snd_payload"),
    "kg_snd_iq_payload_dev": ("test_containment_gpu", "test_snd_iq_payload"),
    "kg_wf_packets_dev": ("test_containment_gpu", "test_wf_packets"),
    "kg_dpump_unpack_dev": ("test_containment_gpu", "test_dpump_unpack"),
    "kg_dpump_unpack_rows_dev": ("test_containment_gpu", "test_dpump_unpack"),
    "kg_fir_process_dev": ("test_containment_gpu", "test_fir_process"),
    "kg_fir_process_each_dev": ("test_containment_gpu", "test_fir_process"),
    "kg_fir_process_taps_dev": ("test_containment_gpu", "test_fir_process_taps"),
    "kg_fir_refilter_dev": ("test_containment_gpu", "test_fir_refilter"),
    "kg_fir_process_spec_dev": ("test_containment_gpu", "test_fir_process_spec"),
    "kg_snd_spec_rows_dev": ("test_containment_gpu", "test_snd_spec_rows"),
    "kg_nb_process_dev": ("test_containment_gpu", "test_nb_process"),
    "kg_math_dev": ("test_containment_gpu", "test_math"),
    "kg_math_atan2f_dev": ("test_containment_gpu", "test_math"),
    "kg_post_process_dev": ("test_containment_post_gpu", "test_post_process"),
    "kg_post_nr_process_dev": ("test_containment_post_gpu", "test_post_nr_process"),
    "kg_post_nrs_process_dev": ("test_containment_post_gpu", "test_post_nrs_process"),
    "kg_post_nbw_process_dev": ("test_containment_post_gpu", "test_post_nbw_process"),
    "kg_post_cfir_process_dev": ("test_containment_post_gpu", "test_post_cfir_process"),
    "kg_post_squelch_perform_dev": ("test_containment_post_gpu", "test_post_squelch_perform"),
    "kg_ddc_wf_push_dev": ("test_containment_ddc_gpu", "test_ddc_wf_push"),
    "kg_ddc_wf_capture_dev": ("test_containment_ddc_gpu", "test_ddc_wf_capture"),
    "kg_ddc_wf_step_dev": ("test_containment_ddc_gpu", "test_ddc_wf_step"),
    "kg_rxddc_push_dev": ("test_containment_ddc_gpu", "test_rxddc_push"),
    "kg_wf_frames_dev": ("test_containment_ddc_gpu", "test_wf_frames"),
    "kg_wf_frames_at_dev": ("test_containment_ddc_gpu", "test_wf_frames"),
    "kg_wf_nb_frames_dev": ("test_containment_ddc_gpu", "test_wf_frames"),
    "kg_aper_update_dev": ("test_containment_ddc_gpu", "test_aper_update"),
    "kg_acq_sample_bits_dev": ("test_containment_ddc_gpu", "test_acq_sample"),
    "kg_acq_sample_iq16_dev": ("test_containment_ddc_gpu", "test_acq_sample"),
    "kg_acq_sample_iq16_batch_dev": ("test_containment_ddc_gpu", "test_acq_sample"),
    "kg_rxbank_step": ("test_containment_bank_gpu", "test_bank_buffers"),      # d_adc in, the bank's own buffers out
}

# entry point -> one-line reason.  Only host-synchronous conveniences without a caller device buffer and the two kg_acq_debug_*
# diagnostics may stand here; today no prototype with a `d_` pointer is either.
EXEMPT = {}


def device_entry_points():
    with open(os.path.join(ROOT, "include", "kiwigpu.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    protos = re.findall(r"\b(kg_\w+)\s*\(([^;{}()]*)\)\s*;", text)
    assert len(protos) > 150, "the header did not parse: %d prototypes" % len(protos)
    return [name for name, args in protos if re.search(r"\bvoid\s*\*\s*d_\w+", args)]


def test_every_device_entry_point_has_a_containment_case():
    names = device_entry_points()
    assert "kg_ddc_wf_push_dev" in names and "kg_rxbank_step" in names and len(names) == len(set(names))
    missing = [n for n in names if n not in REGISTRY and n not in EXEMPT]
    assert not missing, "no containment case for %s: add one (tests/guarded.py) and list it here" % missing
    stale = [n for n in list(REGISTRY) + list(EXEMPT) if n not in names]
    assert not stale, "listed, but no longer a device entry point of the header: %s" % stale
    assert not set(REGISTRY) & set(EXEMPT)
    for n, reason in EXEMPT.items():
        assert reason.strip() and (n.startswith("kg_acq_debug_") or not n.endswith("_dev")), n


def reachable_source(m, fn):
    """the source of m.fn and of the helper functions of the same module that it names (directly or through another helper; never
    another test): what the case can run, not the whole module"""
    seen, todo = {}, [fn]
    while todo:
        f = getattr(m, todo.pop())
        seen[f.__name__] = inspect.getsource(f)
        codes = [f.__code__]
        while codes:
            c = codes.pop()
            codes += [k for k in c.co_consts if inspect.iscode(k)]
            for n in c.co_names + c.co_freevars:
                g = getattr(m, n, None)
                if inspect.isfunction(g) and g.__module__ == m.__name__ and not n.startswith("test_") and n not in seen and n not in todo:
                    todo.append(n)
    return "\n".join(seen.values())


def test_the_registered_cases_exist_and_call_their_entry_point():
    """in the source of the registered test function and of the module's helpers it runs, not anywhere in its module"""
    called = {  # the Python method a case goes through where it does not name the C symbol
        "kg_adpcm_encode_dev": "encode_dev(", "kg_wf_packets_dev": "wf_packets_dev(", "kg_dpump_unpack_rows_dev": "unpack_rows_dev(",
        "kg_fir_process_dev": ".process_dev(", "kg_fir_process_spec_dev": "process_spec_dev(", "kg_snd_spec_rows_dev": "spec_rows_dev(",
        "kg_nb_process_dev": "nb.process_dev(", "kg_post_process_dev": "P.process_dev(", "kg_post_nr_process_dev": "nr_process_dev(",
        "kg_post_nrs_process_dev": "nrs_process_dev(", "kg_post_nbw_process_dev": "nbw_process_dev(", "kg_ddc_wf_push_dev": "d.push_dev(",
        "kg_ddc_wf_capture_dev": "capture_dev(", "kg_rxddc_push_dev": "d.push_dev(", "kg_wf_frames_dev": "frames_dev(",
        "kg_wf_frames_at_dev": "frames_dev(", "kg_wf_nb_frames_dev": "nb_frames(", "kg_aper_update_dev": "update_dev(",
        "kg_acq_sample_bits_dev": "s.sample(", "kg_acq_sample_iq16_dev": "s.sample_iq16(", "kg_acq_sample_iq16_batch_dev": "sample_iq16_batch(",
        "kg_rxbank_step": "bank.step(",
    }
    for name, (mod, fn) in REGISTRY.items():
        m = importlib.import_module("tests." + mod)
        assert callable(getattr(m, fn, None)), (name, mod, fn)
        src = reachable_source(m, fn)
        assert ("." + name + "(") in src or called.get(name, "\0") in src, (name, "is not called in tests/%s.py::%s" % (mod, fn))
