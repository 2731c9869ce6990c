"""Inputs of the noise-blanker scenarios (tests/golden/nb_ref.npz): regenerated from fixed seeds by tools/make_ref_nb_golden.py,
which pinned the reference's outputs for them, and by the tests that replay them.  numpy's PCG64 and float64 arithmetic, rounded
to float32 / int16 once: the same values on every machine."""
import numpy as np


def pulses(n, rng, width, spacing, amp, start=0):
    """impulse noise: bursts of `width` samples every `spacing` samples (jittered), random phase, amplitude `amp`"""
    x = np.zeros(n, np.complex128)
    p = start
    while p < n:
        ph = rng.uniform(0, 2 * np.pi)
        x[p:p + width] += amp * np.exp(1j * (ph + 0.3 * np.arange(min(width, n - p))))
        p += spacing + int(rng.integers(0, max(1, spacing // 4)))
    return x


def audio(kind, n, seed):
    """complex float32 [n, 2]: what snd_service()'s unpack hands the blanker (float samples at int16 scale)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n)
    noise = 300.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    if kind == "noise_pulses":
        x = noise + pulses(n, rng, 3, 700, 9000.0) + pulses(n, rng, 20, 1900, 6000.0, 350) + pulses(n, rng, 60, 2600, 12000.0, 1200)
    elif kind == "carrier_pulses":
        x = 20000.0 * np.exp(2j * np.pi * 0.0371 * t) + 0.3 * noise + pulses(n, rng, 8, 900, 30000.0, 100)
    elif kind == "quiet_then_loud":
        x = 0.01 * noise
        x[n // 2:] += 3000.0 * np.exp(2j * np.pi * 0.011 * t[n // 2:])
        x += pulses(n, rng, 4, 1300, 5000.0, 200)
    else:
        raise ValueError(kind)
    out = np.empty((n, 2), np.float32)
    out[:, 0] = np.round(x.real).clip(-32768, 32767)
    out[:, 1] = np.round(x.imag).clip(-32768, 32767)
    return out


def wf_frames(kind, nframes, seed):
    """int16 [nframes, 8192, 2]: the waterfall DDC's iq_t frames"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = 8192 * nframes
    t = np.arange(n)
    noise = 200.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    if kind == "noise_pulses":
        x = noise + 4000.0 * np.exp(2j * np.pi * 0.123 * t) + pulses(n, rng, 5, 3000, 30000.0, 500)
    elif kind == "silent_loud":
        x = noise.copy()
        x[: 8192 * 2] *= 0.0                       # two silent frames: the flush's drift
        x[8192 * 4: 8192 * 5] *= 40.0
        x += pulses(n, rng, 30, 7000, 25000.0, 100)
    else:
        raise ValueError(kind)
    out = np.empty((nframes, 8192, 2), np.int16)
    out.reshape(-1, 2)[:, 0] = np.round(x.real).clip(-32768, 32767)
    out.reshape(-1, 2)[:, 1] = np.round(x.imag).clip(-32768, 32767)
    return out


def windowed(frames, window):
    """sample_wf(): fi = (float) ii * window[sn] (rx/rx_waterfall.cpp:1054-1061), float32"""
    return (frames.astype(np.float32) * window.astype(np.float32)[None, :, None]).astype(np.float32)
