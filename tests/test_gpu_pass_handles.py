"""The lifecycle that the float32 row passes share (Resampler, MelSpectrogram with either transform, KaldiFeatures): what
last_ms() says before a pass and after a call that launched nothing, one pass through __call__, close() and what a closed
handle answers, the with block, and the one-handle-per-parameter-set cache behind resample, mel_spectrogram and kaldi_fbank.
2 rows of 64 samples per handle; what the passes compute is the matter of the neighbouring test_gpu_*.py files.

No test provokes a fault: a closed handle is refused on the host, before any HIP call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS, T = 2, 64


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


MEL = dict(n_fft=16, hop_length=4, n_mels=4)
MEL_FRAMES = 1 + T // 4  # centred, even n_fft
KALDI_FRAMES = 1 + (T - 16) // 4  # snip_edges

# name -> (a new handle, the documented shape behind [ROWS], the device call with rows = 0, the module entry, its cache)
HANDLES = {
    "resampler": (lambda pkg: pkg.NewResampler(2, 3),
                  (96,),
                  lambda h: h.resample_device(0, T, 0, T, 0, 96),
                  lambda pkg, x: pkg.resample(x, 2, 3),
                  "_RESAMPLERS"),
    "mel": (lambda pkg: pkg.NewMelSpectrogram(16000, **MEL),
            (4, MEL_FRAMES),
            lambda h: h.mel_device(0, T, 0, T, 0, 4 * MEL_FRAMES, MEL_FRAMES),
            lambda pkg, x: pkg.mel_spectrogram(x, 16000, **MEL),
            "_MELS"),
    "mel_fft": (lambda pkg: pkg.NewMelSpectrogram(16000, transform="fft", **MEL),
                (4, MEL_FRAMES),
                lambda h: h.mel_device(0, T, 0, T, 0, 4 * MEL_FRAMES, MEL_FRAMES),
                lambda pkg, x: pkg.mel_spectrogram(x, 16000, transform="fft", **MEL),
                "_MELS"),
    "kaldi": (lambda pkg: pkg.NewKaldiFeatures(16000, 16, 4, num_mel_bins=4, low_freq=20.0),
              (KALDI_FRAMES, 4),
              lambda h: h.features_device(0, T, 0, T, 0, 4 * KALDI_FRAMES, 4),
              lambda pkg, x: pkg.kaldi_fbank(x, 16000, frame_length=1.0, frame_shift=0.25, num_mel_bins=4, low_freq=20.0),
              "_KALDIS"),
}


def rows_of(torch):
    rng = np.random.default_rng(64)
    return torch.from_numpy(rng.uniform(-1.0, 1.0, (ROWS, T)).astype(np.float32)).to("cuda:0")


def assert_closed(h, x):
    """What a closed handle answers: no frames, and ValueError from everything else"""
    assert h.out_frames(T) == 0
    for call in (h.synchronize, h.last_ms, h.plan, lambda: h(x)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("name", list(HANDLES))
def test_lifecycle_of_a_pass_handle(torch, pkg, name):
    new, shape, no_rows, _, _ = HANDLES[name]
    x = rows_of(torch)
    h = new(pkg)
    with pytest.raises(ValueError):
        h.last_ms()  # no pass yet on this handle
    no_rows(h)
    with pytest.raises(ValueError):
        h.last_ms()  # nothing was launched
    out = h(x)
    assert tuple(out.shape) == (ROWS,) + shape and out.dtype is torch.float32 and out.device == x.device
    assert h.out_frames(T) == (shape[0] if name in ("resampler", "kaldi") else shape[1])
    assert h.last_ms() > 0
    h.synchronize()
    assert bool(torch.isfinite(out).all().item())
    h.close()
    h.close()  # a second close is harmless
    assert_closed(h, x)
    with new(pkg) as g:
        assert g.out_frames(T) > 0
    assert_closed(g, x)  # leaving the with block closed it


@pytest.mark.parametrize("name", list(HANDLES))
def test_the_module_entry_keeps_one_handle_per_parameter_set(torch, pkg, name):
    _, shape, _, entry, cache_name = HANDLES[name]
    cache = getattr(pkg, cache_name)
    x = rows_of(torch)
    before = set(cache)
    first = entry(pkg, x)
    added = set(cache) - before
    assert len(added) == 1, "the first call adds exactly one handle"
    handle = cache[next(iter(added))]
    second = entry(pkg, x)
    assert set(cache) - before == added and cache[next(iter(added))] is handle, "the second call adds none"
    assert tuple(first.shape) == (ROWS,) + shape
    assert torch.equal(first.view(torch.int32), second.view(torch.int32)), "the two calls differ"
