"""CPU checks of the sampler's contract: the restatement (tests/_sampler_ref.py) against the published Philox4x32-10 known answers and against softmax, the
collapse rules of sampling.SamplerSettings, and the argument errors of exl3_sample / exl3_gen_feed (reported before any device work)."""
import math
import numpy as np
import pytest
import _sampler_ref as R


def test_philox_known_answers():
    # Random123 kat_vectors: philox4x32 10 rounds
    z = R.philox4x32_10((0, 0, 0, 0), (0, 0))
    assert [int(x) for x in z] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xFFFFFFFF
    o = R.philox4x32_10((f, f, f, f), (f, f))
    assert [int(x) for x in o] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    # vectorised over the first counter word = the scalar result
    v = R.philox4x32_10((np.array([0, f], dtype=np.uint64), np.array([0, f]), np.array([0, f]), np.array([0, f])), (0, 0))
    assert int(v[0][0]) == 0x6627e8d5


def test_uniform_is_exact_in_fp32_and_inside_the_open_interval():
    w = np.array([0, 1, 511, 512, 0xFFFFFFFF, 0x80000000], dtype=np.uint32)
    u = R.uniform(w)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24
    assert np.isfinite(-np.log(-np.log(u))).all()


#: chi-square statistic of the test below (fixed seeds: a constant) and its bar: the 0.999 quantile of chi-square with 15 degrees of freedom
MODE1_CHI2, MODE1_CHI2_BAR = 20.983, 37.70


def test_mode1_frequencies_follow_softmax():
    V, steps, inv_temp, seed = 16, 4000, 0.8, 1234
    l = (np.random.default_rng(7).standard_normal(V) * 1.5).astype(np.float16)
    p = np.exp(l.astype(np.float64) * inv_temp); p /= p.sum()
    counts = np.zeros(V)
    for s in range(steps):
        counts[R.sample(l, 1, inv_temp=inv_temp, row=3, step=s, seed=seed)] += 1
    chi2 = float((((counts - steps * p) ** 2) / (steps * p)).sum())
    assert abs(chi2 - MODE1_CHI2) < 5e-3, chi2
    assert chi2 < MODE1_CHI2_BAR


def test_noise_depends_on_every_counter_word_and_the_seed():
    g = R.gumbel(64, 2, 5, 99)
    assert np.array_equal(g, R.gumbel(64, 2, 5, 99))
    for other in (R.gumbel(64, 3, 5, 99), R.gumbel(64, 2, 6, 99), R.gumbel(64, 2, 5 + (1 << 32), 99), R.gumbel(64, 2, 5, 100), R.gumbel(64, 2, 5, 99 + (1 << 32))):
        assert not np.array_equal(g, other)
    assert np.array_equal(R.gumbel(128, 2, 5, 99)[:64], g)                       # a column's noise does not depend on the row's width


def test_kept_set_definitions():
    l = np.array([1.0, 3.0, 3.0, 2.0, -np.inf, 0.5, 2.0, 2.0], dtype=np.float16)
    assert R.greedy(l) == 1
    assert R.topk_cutoff(l, 1) == 3.0 and R.topk_cutoff(l, 2) == 3.0 and R.topk_cutoff(l, 3) == 2.0 and R.topk_cutoff(l, 100) == 0.5
    assert R.minp_threshold(l, math.log(0.5)) == float(np.float32(3.0) + np.float32(math.log(0.5)))
    # top-p: classes 3 (x2), 2 (x3), 1, 0.5; the top class always stays, a class stays while the cumulative mass is <= p Z
    vals, w, Z = R.masses(l, -np.inf, 1.0)
    assert list(vals) == [3.0, 2.0, 1.0, 0.5]
    assert R.topp_cutoff(l, -np.inf, 0.01, 1.0) == 3.0
    assert R.topp_cutoff(l, -np.inf, float((w[0] + w[1]) / Z) + 1e-6, 1.0) == 2.0
    assert R.topp_cutoff(l, -np.inf, 1.0, 1.0) == 0.5
    assert R.sample(np.array([1.0, np.nan], dtype=np.float16), 0) == -1
    assert R.sample(np.array([1.0, np.inf], dtype=np.float16), 1) == -1
    assert R.sample(np.array([-np.inf, -np.inf], dtype=np.float16), 1) == -1
    assert R.sample(np.array([-np.inf, -2.0], dtype=np.float16), 1, seed=5) == 1


def test_sampler_settings_collapse_rules():
    from exllamav3_amd.sampling import SamplerSettings as S
    assert S(temperature=0.0, top_k=50, top_p=0.9).kernel_args().mode == 0
    assert S(temperature=0.7, top_k=1).kernel_args().mode == 0
    assert S(temperature=0.7, top_p=0.0).kernel_args().mode == 0
    a = S(temperature=0.5, seed=(7 << 32) | 9).kernel_args()
    assert (a.mode, a.filters, a.inv_temp, a.seed) == (1, 0, 2.0, (7 << 32) | 9)
    a = S(temperature=0.5, top_k=0, top_p=1.0, min_p=0.0).kernel_args()
    assert a.mode == 1                                                           # every filter at its neutral value drops its bit
    # min-p alone: mode 2; ln(min_p) when min-p comes before temperature, T * ln(min_p) when temperature comes first
    a = S(temperature=0.5, min_p=0.1, temperature_last=True).kernel_args()
    assert a.mode == 2 and a.minp_log == pytest.approx(math.log(0.1))
    a = S(temperature=0.5, min_p=0.1).kernel_args()
    assert a.mode == 2 and a.minp_log == pytest.approx(0.5 * math.log(0.1))
    # filters: mode 3 with the reference's flag bits (1 top-k, 2 top-p, 4 min-p); the filter temperature is T only when temperature comes first
    a = S(temperature=0.8, top_k=50, top_p=0.9).kernel_args()
    assert (a.mode, a.filters, a.top_k) == (3, 3, 50) and a.top_p == pytest.approx(0.9) and a.inv_temp == a.inv_temp_filter == pytest.approx(1.25)
    a = S(temperature=0.8, top_k=50, top_p=0.9, min_p=0.05, temperature_last=True).kernel_args()
    assert (a.mode, a.filters) == (3, 7) and a.inv_temp_filter == 1.0 and a.inv_temp == pytest.approx(1.25) and a.minp_log == pytest.approx(math.log(0.05))
    assert S(temperature=1.0, top_p=0.9).kernel_args().filters == 2 and S(temperature=1.0, top_k=40, min_p=0.1).kernel_args().filters == 5
    with pytest.raises(ValueError):
        S(temperature=-1.0).kernel_args()
    with pytest.raises(ValueError):
        S(top_p=1.5).kernel_args()


def test_sampler_names_of_the_reference_are_not_exported():
    """The reference's sampler ops would promise curand's noise sequence; the device sampler lives in exllamav3_amd.sampling under its own names."""
    from exllamav3_amd import ext
    for name in ("argmax_sample", "gumbel_sample", "fused_sampler", "gumbel_noise_f16", "gumbel_noise_f32", "gumbel_noise_log"):
        assert name not in vars(ext), name


def test_sample_and_feed_argument_errors_are_reported_without_gpu():
    from exllamav3_amd import _lib, sampling
    l = _lib.lib()
    assert sampling.workspace_bytes(1) > 0 and sampling.workspace_bytes(16) == 16 * sampling.workspace_bytes(1)
    with pytest.raises(RuntimeError):
        sampling.workspace_bytes(17)
    A = 4096                                                                     # (an aligned non-null address: never dereferenced, the checks come first)
    S = lambda *a: l.exl3_sample(*a)
    #          logits m  ld   size mode filt k  p    it   itf  mpl  seed  step row0 ws bytes     tokens cut kept stream
    assert S(A, 0, 128, 128, 0, 0, 0, 1.0, 1.0, 1.0, 0.0, 0, 0, None, 0, A, 1 << 20, A, None, None, None) == -1 and b"m must be in [1, 16]" in l.exl3_last_error()
    assert S(A, 17, 128, 128, 0, 0, 0, 1.0, 1.0, 1.0, 0.0, 0, 0, None, 0, A, 1 << 20, A, None, None, None) == -1
    assert S(A, 1, 100, 100, 0, 0, 0, 1.0, 1.0, 1.0, 0.0, 0, 0, None, 0, A, 1 << 20, A, None, None, None) == -1 and b"multiple of 8" in l.exl3_last_error()
    assert S(A, 1, 128, 129, 0, 0, 0, 1.0, 1.0, 1.0, 0.0, 0, 0, None, 0, A, 1 << 20, A, None, None, None) == -1
    assert S(A, 1, 128, 128, 4, 0, 0, 1.0, 1.0, 1.0, 0.0, 0, 0, None, 0, A, 1 << 20, A, None, None, None) == -1 and b"mode must be in [0, 3]" in l.exl3_last_error()
    assert S(None, 1, 128, 128, 0, 0, 0, 1.0, 1.0, 1.0, 0.0, 0, 0, None, 0, A, 1 << 20, A, None, None, None) == -1 and b"null pointer" in l.exl3_last_error()
    assert S(A + 2, 1, 128, 128, 0, 0, 0, 1.0, 1.0, 1.0, 0.0, 0, 0, None, 0, A, 1 << 20, A, None, None, None) == -1 and b"16-byte aligned" in l.exl3_last_error()
    assert S(A, 2, 128, 128, 0, 0, 0, 1.0, 1.0, 1.0, 0.0, 0, 0, None, 0, A, 4096, A, None, None, None) == -1 and b"workspace too small" in l.exl3_last_error()
    assert S(A, 1, 128, 128, 1, 0, 0, 1.0, 0.0, 1.0, 0.0, 0, 0, None, 0, A, 1 << 20, A, None, None, None) == -1 and b"inv_temp must be positive" in l.exl3_last_error()
    assert S(A, 1, 128, 128, 3, 0, 0, 1.0, 1.0, 1.0, 0.0, 0, 0, None, 0, A, 1 << 20, A, None, None, None) == -1 and b"needs filter bits" in l.exl3_last_error()
    assert S(A, 1, 128, 128, 3, 1, 0, 1.0, 1.0, 1.0, 0.0, 0, 0, None, 0, A, 1 << 20, A, None, None, None) == -1 and b"top_k must be at least 1" in l.exl3_last_error()
    assert S(A, 1, 128, 128, 3, 2, 0, 1.5, 1.0, 1.0, 0.0, 0, 0, None, 0, A, 1 << 20, A, None, None, None) == -1 and b"top_p must be in (0, 1]" in l.exl3_last_error()
    assert S(A, 1, 128, 128, 2, 0, 0, 1.0, 1.0, 1.0, 0.5, 0, 0, None, 0, A, 1 << 20, A, None, None, None) == -1 and b"minp_log must not be positive" in l.exl3_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(-1)
    F = lambda *a: l.exl3_gen_feed(*a)
    #          sampled forced flen m  embed vocab hidden x0 out olen pos seq att inv step stream
    assert F(A, None, 0, 0, A, 10, 64, A, None, 0, None, None, None, A, A, None) == -1 and b"m must be in [1, 16]" in l.exl3_last_error()
    assert F(A, None, 0, 1, None, 10, 64, A, None, 0, None, None, None, A, A, None) == -1 and b"null pointer" in l.exl3_last_error()
    assert F(None, None, 0, 1, A, 10, 64, A, None, 0, None, None, None, A, A, None) == -1 and b"sampled or forced" in l.exl3_last_error()
    assert F(A, None, 0, 1, A, 10, 60, A, None, 0, None, None, None, A, A, None) == -1 and b"multiple of 8" in l.exl3_last_error()
    assert F(A, None, 0, 1, A, 10, 64, A + 8, None, 0, None, None, None, A, A, None) == -1 and b"16-byte aligned" in l.exl3_last_error()
    assert F(A, A, 0, 1, A, 10, 64, A, None, 0, None, None, None, A, A, None) == -1 and b"forced_len" in l.exl3_last_error()
    assert F(A, None, 0, 1, A, 10, 64, A, A, 0, None, None, None, A, A, None) == -1 and b"out_len" in l.exl3_last_error()
