"""The measurement channel's row program, built for the host (tests/hostsim_channel), against its NumPy statement
(tests/channel_ref.py), fp64.

Bounds.  Noise on a pass-through channel: 256 eps sigma absolute - the rounded argument 2 pi u2 carries at most 4 pi eps,
cos adds about 2 eps, sqrt(-2 ln u1) <= 8.6: about 125 eps, doubled.  (The inputs are kept below 4 sigma, so that the last
rounding of v, which the fma of the row program and the two roundings of NumPy may do differently, stays inside it.)
Transparent, quantised and delayed outputs: bit for bit.  The difference output: 1e-12 of the largest |g| - a few
roundings per tick, with fma against NumPy's two roundings."""
import numpy as np
import pytest

from tests import channel_ref, hostsim_channel

EPS = np.finfo(np.float64).eps
STAT_SEED, STAT_ROWS, STAT_COLS, STAT_TICKS = 20261019, 4096, 6, 16


def test_philox_known_answers():
    h = lambda w: " ".join(f"{int(x):08x}" for x in w)
    cases = [((0,) * 4, (0,) * 2, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
              "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in cases:
        assert h(hostsim_channel.philox(counter, key)) == want
        assert h(channel_ref.philox4x32(counter, key)) == want


def test_normal_known_answer():
    want_words, want_n = [142777083, 145619647, 2157388349, 3412851148], -2.608907907505362
    w, n = hostsim_channel.normal(7, 5, 3, 2)
    assert w.tolist() == want_words and [int(x) for x in channel_ref.words(7, 5, 3, 2)] == want_words
    assert abs(float(channel_ref.normal(7, 5, 3, 2)) - want_n) <= 256 * EPS
    assert abs(n - want_n) <= 256 * EPS
    # a row number past 2^32 and a negative one use the high word
    for row in (5 + (1 << 32), -1):
        w, n = hostsim_channel.normal(7, row, 3, 2)
        assert w.tolist() == [int(x) for x in channel_ref.words(7, row, 3, 2)] and w.tolist() != want_words
        assert abs(n - float(channel_ref.normal(7, row, 3, 2))) <= 256 * EPS


def _run(kw, xs, B, W, resets=()):
    """the same ticks through the host build and the reference -> (host outs, host dys, ref outs, ref dys, ref)"""
    host, ref = hostsim_channel.HostChannel(W, B, **kw), channel_ref.ChannelRef(W, B, **kw)
    ho, hd, ro, rd = [], [], [], []
    for t, x in enumerate(xs):
        if t in resets:
            host.counter[resets[t]] = 0
            ref.counter[resets[t]] = 0
        o, d = host.tick(x)
        ho.append(o), hd.append(d)
        o, d = ref.tick(x)
        ro.append(o), rd.append(d)
    assert np.array_equal(host.counter, ref.counter)
    return np.array(ho), hd, np.array(ro), rd, ref


def test_noise_on_a_pass_through_channel():
    B, W, K = 37, 7, 8
    sigma = np.array([0.5, 0.01, 0.0, 2.0, 1e-3, 0.0, 0.1])
    rng = np.random.RandomState(1)
    xs = rng.uniform(-2, 2, (K, B, W)) * np.where(sigma > 0, sigma, 1.0)
    ho, _, ro, _, _ = _run(dict(sigma=sigma, seed=11, row_offset=1 << 33), xs, B, W)
    err = np.abs(ho - ro).max(axis=(0, 1))
    print("largest error in eps sigma per column:", err[sigma > 0] / (EPS * sigma[sigma > 0]))
    assert (err[sigma > 0] <= 256 * EPS * sigma[sigma > 0]).all()
    assert np.array_equal(ho[:, :, sigma == 0], xs[:, :, sigma == 0])  # no number is drawn there
    assert np.abs(ro - xs)[:, :, sigma > 0].min() > 0


def test_transparent_channel_is_the_identity_bit_for_bit():
    B, W = 5, 16
    xs = np.random.RandomState(2).standard_normal((3, B, W)) * 10.0 ** np.arange(-8, 8)
    host = hostsim_channel.HostChannel(W, B, seed=3, w0=9)
    for x in xs:
        out, dy = host.tick(x)
        assert dy is None and out.tobytes() == x.tobytes()
    assert host.counter.tolist() == [3] * B


def test_quantisation_without_noise_is_exact_and_ties_go_to_even():
    B, W, K = 6, 4, 3
    res = np.array([0.25, 2 * np.pi / 2 ** 14, 0.0, 1e-3])
    bias = np.array([0.0, 0.01, 0.5, 0.0])
    xs = np.random.RandomState(3).uniform(-3, 3, (K, B, W))
    xs[0, :, 0] = np.array([2.5, 3.5, -2.5, -3.5, 0.5, -0.5]) * 0.25  # exact ties of a power-of-two resolution
    ho, _, ro, _, _ = _run(dict(resolution=res, bias=bias), xs, B, W)
    assert ho.tobytes() == ro.tobytes()
    assert np.array_equal(ho[0, :, 0], np.array([2.0, 4.0, -2.0, -4.0, 0.0, 0.0]) * 0.25)
    for c in np.nonzero(res)[0]:
        k = ho[:, :, c] / res[c]
        assert np.array_equal(np.rint(k) * res[c], ho[:, :, c]), c
    assert np.array_equal(ho[:, :, 2], xs[:, :, 2] + 0.5)


@pytest.mark.parametrize("delay", [0, 1, 3])
def test_delay_returns_the_sample_of_tick_t_minus_d(delay):
    B, W, K = 9, 5, 8
    xs = np.random.RandomState(4).uniform(-1, 1, (K, B, W))
    kw = dict(delay=delay, resolution=[0.0, 1e-3, 0.0, 0.5, 0.0], sigma=[0.2, 0.0, 0.0, 0.2, 0.0], seed=5)
    # the undelayed samples of the reference: v of tick t
    _, _, v, _, _ = _run(dict(kw, delay=0), xs, B, W)
    ho, _, ro, _, _ = _run(kw, xs, B, W)
    quiet = [1, 2, 4]  # columns without noise: bit for bit; the noisy ones within the noise bound
    for t in range(K):
        assert np.array_equal(ro[t], v[max(t - delay, 0)])
        assert np.array_equal(ho[t][:, quiet], v[max(t - delay, 0)][:, quiet])
    assert np.abs(ho - ro).max() <= 256 * EPS * 0.2
    # a zero-filled counter in the middle of a run: rows 2..5 start again at tick 5 - their own tick numbers, their own
    # first sample held; the other rows go on
    rows = slice(2, 6)
    ho, _, ro, _, _ = _run(dict(kw, sigma=0.0), xs, B, W, resets={5: rows})
    _, _, v, _, _ = _run(dict(kw, sigma=0.0, delay=0), xs, B, W)
    assert ho.tobytes() == ro.tobytes()
    for t in range(K):
        src = np.full(B, max(t - delay, 0))
        if t >= 5:
            src[rows] = max(t - delay, 5)
        assert np.array_equal(ho[t], v[src, np.arange(B)]), t


@pytest.mark.parametrize("tau_diff", [0.0, 0.005])
@pytest.mark.parametrize("delay", [0, 2])
def test_difference_output(delay, tau_diff):
    B, W, K = 11, 6, 16
    rng = np.random.RandomState(6)
    xs = np.cumsum(rng.uniform(-1e-3, 1e-3, (K, B, W)), axis=0) + rng.uniform(-1, 1, (B, W))
    kw = dict(delay=delay, difference=True, tau_diff=tau_diff, dt=0.001, resolution=2 * np.pi / 2 ** 14)
    host, ref = hostsim_channel.HostChannel(W, B, **kw), channel_ref.ChannelRef(W, B, **kw)
    gmax, err = 0.0, 0.0
    for t, x in enumerate(xs):
        (ho, hd), (ro, rd) = host.tick(x), ref.tick(x)
        assert ho.tobytes() == ro.tobytes()
        if t == 0:
            assert not hd.any()
        gmax = max(gmax, np.abs(ref.g).max())
        err = max(err, np.abs(hd - rd).max())
        if tau_diff == 0 and t > 0:  # a = 1: the plain difference quotient, up to the fma's single rounding
            assert np.abs(hd - ref.g).max() <= 4 * EPS * gmax
    print(f"largest |g| {gmax:.3e}, largest error of dy {err:.3e}")
    assert gmax > 0 and err <= 1e-12 * gmax


def test_statistics_of_the_reference_normals():
    n = channel_ref.normal_block(STAT_SEED, np.arange(STAT_ROWS), np.arange(STAT_TICKS), np.arange(STAT_COLS))
    assert n.size == 393216
    z = channel_ref.statistics(n)
    print({k: round(float(v), 2) for k, v in z.items()})
    assert all(abs(v) <= 4 for v in z.values()), z
    # the host build draws the same numbers: sigma = 1 on a zero input, rows 0..4095, 16 ticks
    host = hostsim_channel.HostChannel(STAT_COLS, STAT_ROWS, sigma=1.0, seed=STAT_SEED)
    zero = np.zeros((STAT_ROWS, STAT_COLS))
    got = np.stack([host.tick(zero)[0] for _ in range(STAT_TICKS)], axis=1)
    assert np.abs(got - n).max() <= 256 * EPS
    assert all(abs(v) <= 4 for v in channel_ref.statistics(got).values())
