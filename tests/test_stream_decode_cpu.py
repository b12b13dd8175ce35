"""CPU: the stream kernel's entry decode (rt_stream_decode).

stream_entry turns a queue entry e into (frame, live pixel, sample) with two
multiply-highs by magic numbers that render_stream computes per launch
(rt_internal.h stream_decode / stream_div_of).  rt_stream_decode runs that same
function on the host with the same magic numbers; here it is held to Python's
divmod for both entry orders, for divisors from 1 to 2^24 (powers of two, their
neighbours, 65535 / 65537) and for the entries at which a wrong magic number
shows first: 0, 1, around every divisor and its multiples, and the largest
entry a launch can hold (2^31 - 1 is the bound on its entry count).
"""
import itertools

import numpy as np
import pytest

import rtgo

E_MAX = (1 << 31) - 1  # entries of a launch: fewer than 2^31
DIVISORS = [1, 2, 3, 7, 16, 25, 100, 255, 65535, 65537]
NLIVE = [1, 2, 3, 7, 16, 25, 100, 255, 65535, 65537, 480000, (1 << 24) - 1, 1 << 24]


def _entries(divs):
    """0, 1, d - 1, d, d + 1 of every divisor and product of divisors, multiples
    of them +- 1 up to the bound, and the largest entry."""
    es = {0, 1, E_MAX, E_MAX - 1}
    prods = set(divs) | {a * b for a, b in itertools.combinations(divs, 2)} | {int(np.prod(divs))}
    for d in prods:
        for m in (1, 2, 3, 5, 1000, 65535, 65536, 65537, E_MAX // d, E_MAX // d - 1):
            for delta in (-1, 0, 1):
                es.add(m * d + delta)
    return np.array(sorted(e for e in es if 0 <= e <= E_MAX), np.uint32)


def _want(order, frames, nlive, spp, e):
    e = int(e)
    if order == 0:  # e = (fl * nlive + i) * spp + s
        t, s = divmod(e, spp)
        fl, i = divmod(t, nlive)
    else:  # e = (i * spp + s) * frames + fl
        t, fl = divmod(e, frames)
        i, s = divmod(t, spp)
    return fl, i, s


def _hold(order, frames, nlive, spp):
    es = _entries((frames, nlive, spp))
    got = rtgo.stream_decode(order, frames, nlive, spp, es)
    assert got.shape == (len(es), 3)
    want = np.array([_want(order, frames, nlive, spp, e) for e in es], np.uint64)
    bad = np.nonzero((got.astype(np.uint64) != want).any(axis=1))[0]
    assert bad.size == 0, (order, frames, nlive, spp, int(es[bad[0]]), got[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("spp", DIVISORS)
@pytest.mark.parametrize("frames", DIVISORS)
def test_frames_and_samples(order, frames, spp):
    """Every pair of the listed divisors as (frames, spp), with a small, an odd
    and a 2^24 live-pixel count."""
    for nlive in (1, 480000, 1 << 24):
        _hold(order, frames, nlive, spp)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("nlive", NLIVE)
def test_live_pixels(order, nlive):
    for frames, spp in ((1, 1), (3, 7), (25, 100), (32, 750)):
        _hold(order, frames, nlive, spp)


@pytest.mark.parametrize("order", [0, 1])
def test_random_entries_of_the_headline_launch(order):
    """The bench's launch (25 frames, 100 samples) at a live-pixel count of its
    size: 10^5 random entries and the launch's last ones."""
    frames, nlive, spp = 25, 238733, 100
    total = frames * nlive * spp
    rng = np.random.default_rng(7)
    es = np.concatenate([rng.integers(0, total, 100000), np.arange(total - 1000, total)]).astype(np.uint32)
    got = rtgo.stream_decode(order, frames, nlive, spp, es).astype(np.int64)
    e = es.astype(np.int64)
    if order == 0:
        want = np.stack([e // spp // nlive, e // spp % nlive, e % spp], axis=1)
    else:
        want = np.stack([e % frames, e // frames // spp, e // frames % spp], axis=1)
    assert (got == want).all()
    # the decoded triple is the entry again, and within the launch
    back = (got[:, 0] * nlive + got[:, 1]) * spp + got[:, 2] if order == 0 else \
        (got[:, 1] * spp + got[:, 2]) * frames + got[:, 0]
    assert (back == e).all() and (got[:, 0] < frames).all() and (got[:, 1] < nlive).all() and (got[:, 2] < spp).all()


def test_every_divisor_up_to_4096_at_the_bound():
    """d = 1 .. 4096 as the first divisor: the entries around the largest
    multiple of d below 2^31, where a magic number one too small fails first."""
    for d in range(1, 4097):
        top = E_MAX // d * d
        es = np.array(sorted({0, d - 1, d, top - 1, top, min(top + d - 1, E_MAX), E_MAX}), np.uint32)
        got = rtgo.stream_decode(0, 1, 1, d, es).astype(np.int64)
        e = es.astype(np.int64)
        assert (got[:, 2] == e % d).all() and (got[:, 0] == e // d).all() and (got[:, 1] == 0).all(), d


def test_refused_arguments():
    import ctypes

    u32p = ctypes.POINTER(ctypes.c_uint32)
    e = np.array([5], np.uint32)
    out = np.zeros(3, np.uint32)

    def call(order, frames, nlive, spp, entries=e):
        return rtgo.lib().rt_stream_decode(order, frames, nlive, spp, entries.ctypes.data_as(u32p), entries.size,
                                           out.ctypes.data_as(u32p))

    assert call(0, 2, 3, 4) == rtgo.RT_OK and out.tolist() == [0, 1, 1]
    assert call(2, 2, 3, 4) != rtgo.RT_OK
    assert call(0, 0, 3, 4) != rtgo.RT_OK and call(0, 2, 0, 4) != rtgo.RT_OK and call(0, 2, 3, 0) != rtgo.RT_OK
    assert call(0, 1 << 31, 3, 4) != rtgo.RT_OK
    assert call(0, 2, 3, 4, np.array([1 << 31], np.uint32)) != rtgo.RT_OK
    assert rtgo.lib().rt_stream_decode(0, 2, 3, 4, None, 1, out.ctypes.data_as(u32p)) != rtgo.RT_OK
