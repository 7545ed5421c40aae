"""tests/dropout_reference.py pinned on the host, so that a mistake in it is not read as a kernel bug: known answers and edge
keys of the generator text in include/tfgnn.h, and the statistics of the reference's own stream on fixed inputs.

Statistics.  A case is one (rate, seed, epoch); its stream is the keep decision of flat elements 0 .. 2^24 - 1 (2^22 groups of
four).  Every statistic is held to 5 sigma of its null:
  * kept elements per lane position e = 0..3: binomial(2^22, p) with p = 1 - threshold / 2^24 EXACTLY (the element's 24-bit number
    is uniform);
  * product-moment correlation r of two 0/1 sequences of n pairs: sigma = 1 / sqrt(n) - lags 4, 8, 64, 320 and 1280 inside a
    stream, and between the streams of two seeds / two epochs over 2^22 elements (the seeds consecutive integers, as the layer
    stack forms them: dropout_seed * 1000003 + call number).

Lane pairs inside a group are the one exception, by design.  Write the group's word as four bytes D0 D1 D2 D3 (top first): the
number of element e is the three bytes D[e] D[e+1] D[e+2] (indices mod 4), so its decision hangs on D[e] - a byte no other element
decides on - unless D[e] equals the threshold's top byte t.  With T = t * 2^16 + lo:
    K_e = A_e + R_e,   A_e = [D[e] > t],   R_e = [D[e] = t] [D[e+1] D[e+2] >= lo],   P(D[e] = t) = 2^-8.
For a uniform word the A_e are independent, so Cov(K_a, K_b) = Cov(A_a, R_b) + Cov(R_a, A_b) + Cov(R_a, R_b).  Take b = a + 1: R_b
reads D[a+2], D[a+3], not D[a], so Cov(A_a, R_b) = 0; R_a reads D[b] as the TOP byte of its 16-bit number:
    Cov(R_a, A_b) = 2^-8 Cov([D[b] D[b+1] >= lo], [D[b] > t])  (law of total covariance over the event D[a] = t; outside it R_a = 0).
Both indicators increase in the one byte D[b]; for two increasing threshold events of probabilities s <= l on one variable the
covariance is s (1 - l), and with one of them [D[b] > t] of probability p' that is at most p' (1 - p') = Var A_b.  Var A_b and
Var K_a = Var K_b = p (1 - p) differ by a factor within 2^-8 of one, hence
    |corr(K_a, K_a+1)| <= 2^-8 (1 + O(2^-8)) + |Cov(R_a, R_b)| / (p (1 - p)),
and the last term carries P(D[a] = t, D[b] = t) = 2^-16.  For b = a + 2 each of R_a, R_b reads the other's deciding byte only as
the LOW byte of its 16-bit number, which matters only when the byte above equals lo's top byte: every term carries 2^-16.  The
2^-16 terms are divided by p (1 - p), so "2^-8 + 2^-15" is a statement about the rates of this file, not about every rate:
``exact_lane_correlation`` enumerates the population value for a uniform word (exactly, in integers: given the two bytes both
elements read, their decisions hang on two different free bytes and are independent) and the test holds it to that bound before
the sample is looked at.  The sample (2^22 pairs: 5 sigma = 0.0024 < 2^-8 = 0.0039, so the bound bites) is held to
2^-8 + 2^-15 + 5 sigma, and to 5 sigma around the exact value.  At rates whose threshold has sixteen zero low bits (0.5, 0.25,
0.125) lo = 0, R_e = [D[e] = t], K_e = [D[e] >= t]: the lanes are exactly independent and get plain 5 sigma."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import dropout_reference as ref
from tests.neighbor_sample_reference import M32, M64, lowbias32, lowbias32_many

N = 1 << 24          # elements of a per-case stream
N_PAIR = 1 << 22     # elements of a stream compared with another stream
SIGMAS = 5.0
STACK = 7 * 1000003  # seeds as the stack forms them: dropout_seed * 1000003 + call number
TOP_RATE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))  # the largest float32 below 1

# every rate, seed and epoch of the sets once; the last two are the stack's seeds at the exactly independent rates
CASES = [(0.003, 0, 0), (0.05, 1, 1), (0.1, 2, 2), (0.2, 1000003, 3), (0.5, 1000004, 7), (0.9, 1 << 63, M32), (0.1, M64, 0),
         (0.25, STACK + 1, 0), (0.125, STACK + 2, 1)]
INDEPENDENT_RATES = (0.5, 0.25, 0.125)
SEED_PAIRS = [(0, 1), (1, 2), (1000003, 1000004), (1 << 63, M64), (STACK + 1, STACK + 2), (STACK + 2, STACK + 3)]
EPOCH_PAIRS = [(0, 1), (1, 2), (2, 3), (3, 7), (M32, 0)]
LAGS = (4, 8, 64, 320, 1280)


@functools.lru_cache(maxsize=None)
def _stream(rate, seed, epoch, n=N):
    k = ref.keep(seed, rate, epoch, 0, n)
    k.setflags(write=False)
    return k


def _corr(a, b):
    """product-moment correlation of two bool arrays, from exact counts"""
    n = a.size
    na, nb, nab = int(np.count_nonzero(a)), int(np.count_nonzero(b)), int(np.count_nonzero(a & b))
    return (n * nab - na * nb) / math.sqrt(na * (n - na) * nb * (n - nb))


def _inverse_lowbias32(x):
    x ^= x >> 16
    x = (x * 0x43021123) & M32
    x ^= (x >> 15) ^ (x >> 30)
    x = (x * 0x1D69E2A5) & M32
    x ^= x >> 16
    return x


def _keep_one(seed, rate, epoch, idx):
    """one element, in plain integers, read off include/tfgnn.h a second time"""
    z = (seed + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    s0, s1 = z & M32, z >> 32
    if epoch:
        s0 ^= lowbias32((epoch * 0x9E3779B9 + 0x7F4A7C15) & M32)
        s1 = (s1 + epoch * 0x85EBCA6B) & M32
    group, e = idx >> 2, idx & 3
    if group >> 32:
        s0 ^= lowbias32(((group >> 32) * 0x9E3779B9 + 1) & M32)
    w = lowbias32((group & M32) ^ s0) ^ s1
    u24 = (((w << (8 * e)) | (w >> (32 - 8 * e))) & M32) >> 8
    t = Fraction(float(np.float32(rate))) * (1 << 24)
    return u24 >= math.ceil(t)


# ---- known answers and edge keys ----------------------------------------------------------------------------------------
def test_key_words_of_seed_zero_are_splitmix64s_first_output():
    k = ref.key(0, 0.1, 0)
    assert (k.s1 << 32 | k.s0) == 0xE220A8397B1DCDAF
    assert (k.s0, k.s1) == (0x7B1DCDAF, 0xE220A839)


def test_lowbias32_is_undone_by_its_inverse():
    rng = np.random.default_rng(1)
    words = [int(x) for x in rng.integers(0, 1 << 32, size=10000, dtype=np.uint64)] + [0, 1, M32]
    assert all(_inverse_lowbias32(lowbias32(x)) == x for x in words)
    assert np.array_equal(lowbias32_many(np.array(words, dtype=np.uint64)), np.array([lowbias32(x) for x in words], dtype=np.uint64))
    assert lowbias32(0) == 0 and lowbias32(1) != 1


@pytest.mark.parametrize("rate,threshold,scale", [
    (0.0, 0, 1.0), (2.0 ** -24, 1, 1.0 / (1.0 - 2.0 ** -24)), (0.1, 0x19999A, None), (0.2, 0x333334, None), (0.5, 0x800000, 2.0),
    (0.25, 0x400000, None), (0.125, 0x200000, 8.0 / 7.0), (TOP_RATE, (1 << 24) - 1, 2.0 ** 24)])
def test_threshold_and_scale(rate, threshold, scale):
    k = ref.key(3, rate, 0)
    assert k.threshold == threshold
    assert k.scale.dtype == np.float32
    r32 = np.float32(rate)
    assert k.scale == np.float32(1.0) / (np.float32(1.0) - r32)
    if scale is not None:
        assert k.scale == np.float32(scale)
    # the threshold is the smallest integer that is not below rate * 2^24 (of the float32 rate)
    exact = Fraction(float(r32)) * (1 << 24)
    assert threshold - 1 < exact <= threshold


def test_threshold_is_taken_of_the_float32_rate():
    # 0.1 as a double is below the float32 0.1: both round up to the same integer here, 0.3 tells them apart on the scale
    assert ref.threshold(0.1) == math.ceil(Fraction(float(np.float32(0.1))) * (1 << 24)) == 0x19999A
    assert ref.threshold(0.7) == math.ceil(Fraction(float(np.float32(0.7))) * (1 << 24))
    assert ref.scale(0.3) == np.float32(1.0) / (np.float32(1.0) - np.float32(0.3))


def test_rate_zero_keeps_everything_with_scale_one():
    assert ref.keep(12345, 0.0, 0, 0, 4096).all() and ref.keep(M64, 0.0, 9, 5, 4096).all()
    m = ref.mask((7, 9), 0.0, 3)
    assert m.dtype == np.float32 and m.shape == (7, 9) and (m == 1.0).all()


def test_top_rate_keeps_only_the_all_ones_number():
    kept = ref.keep(11, TOP_RATE, 0, 0, 1 << 20)
    numbers = ref.lane_numbers(ref.group_words(ref.key(11, TOP_RATE, 0), 0, 1 << 18)).reshape(-1)
    assert np.array_equal(kept, numbers == 0xFFFFFF)
    assert ref.mask(8, TOP_RATE, 11).max() in (0.0, 2.0 ** 24)


def test_element_e_takes_the_word_rotated_left_by_8e_bits():
    got = ref.lane_numbers(np.array([0x11223344, 0x80000001], dtype=np.uint32))
    assert got.tolist() == [[0x112233, 0x223344, 0x334411, 0x441122], [0x800000, 0x000001, 0x000180, 0x018000]]


def test_kept_means_not_below_the_threshold():
    k = ref.key(21, 0.2, 0)
    numbers = ref.lane_numbers(ref.group_words(k, 0, 1 << 16)).reshape(-1)
    kept = ref.keep(21, 0.2, 0, 0, 1 << 18)
    assert np.array_equal(kept, numbers >= 0x333334)
    assert kept.mean() > 0.75
    m = ref.mask(1 << 18, 0.2, 21)
    assert np.array_equal(m != 0, kept) and set(np.unique(m).tolist()) == {0.0, float(k.scale)}


def test_epoch_step():
    base = ref.key(0, 0.1, 0)
    for e in (1, 2, 7, M32):
        k = ref.key(0, 0.1, e)
        assert k.s0 == base.s0 ^ lowbias32((e * 0x9E3779B9 + 0x7F4A7C15) & M32)
        assert k.s1 == (base.s1 + e * 0x85EBCA6B) & M32
        assert (k.threshold, k.scale) == (base.threshold, base.scale)
    assert ref.key(0, 0.1, 1).s1 == 0x680C72A4  # 0xE220A839 + 0x85EBCA6B, carried out by hand
    assert ref.key(0, 0.1, 1 << 32) == base  # the epoch is a 32-bit word
    assert not np.array_equal(ref.keep(0, 0.1, 0, 0, 4096), ref.keep(0, 0.1, 1, 0, 4096))


def test_high_word_term_changes_group_2_32_and_leaves_the_group_before_alone():
    k = ref.key(5, 0.1, 0)
    words = ref.group_words(k, (1 << 32) - 1, 2)
    assert int(words[0]) == lowbias32(M32 ^ k.s0) ^ k.s1
    assert int(words[1]) == lowbias32(0 ^ k.s0 ^ lowbias32(0x9E3779B9 + 1)) ^ k.s1
    assert int(words[1]) != lowbias32(0 ^ k.s0) ^ k.s1 == int(ref.group_words(k, 0, 1)[0])
    far = ref.group_words(k, 3 << 32 | 17, 1)
    assert int(far[0]) == lowbias32(17 ^ k.s0 ^ lowbias32((3 * 0x9E3779B9 + 1) & M32)) ^ k.s1


def test_array_form_equals_the_element_form_at_any_start():
    rng = np.random.default_rng(2)
    for rate, seed, epoch in [(0.1, 2, 0), (0.2, STACK + 1, 3), (0.9, M64, M32), (0.003, 1 << 63, 1)]:
        for start in (0, 1, 2, 3, 5, (1 << 34) - 6, (1 << 36) + 1, int(rng.integers(1, 1 << 40))):
            got = ref.keep(seed, rate, epoch, start, 13)
            assert got.tolist() == [_keep_one(seed, rate, epoch, start + i) for i in range(13)], (rate, seed, epoch, start)
    whole = ref.keep(9, 0.5, 2, 0, 64)
    assert all(np.array_equal(ref.keep(9, 0.5, 2, s, n), whole[s:s + n]) for s in range(9) for n in (0, 1, 4, 7, 55))
    assert ref.mask((3, 5), 0.5, 9, 2).reshape(-1).tolist() == [2.0 if k else 0.0 for k in whole[:15]]


# ---- the scale matches the keep probability -----------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0.003, 0.05, 0.1, 0.2, 0.25, 0.125, 0.5, 0.9, 2.0 ** -24, TOP_RATE])
def test_kept_values_are_unbiased_within_float32_rounding(rate):
    """E[mask] = P(keep) * scale = (1 - threshold / 2^24) * scale is 1 within 2^-23 / (1 - rate): the ceiling moves P(keep) by less
    than 2^-24, the float32 subtraction is exact for these rates or rounds by <= 2^-25, and the division rounds by 2^-24 relative."""
    k = ref.key(0, rate, 0)
    r = Fraction(float(np.float32(rate)))
    mean = (1 - Fraction(k.threshold, 1 << 24)) * Fraction(float(k.scale))
    assert abs(mean - 1) <= Fraction(1, 1 << 23) / (1 - r), float(mean - 1)


# ---- statistics of the stream ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,seed,epoch", CASES)
def test_keep_fraction_per_lane(rate, seed, epoch):
    lanes = _stream(rate, seed, epoch).reshape(-1, 4)
    groups = lanes.shape[0]
    p = 1 - ref.threshold(rate) / (1 << 24)
    sigma = math.sqrt(groups * p * (1 - p))
    for e in range(4):
        z = (int(np.count_nonzero(lanes[:, e])) - groups * p) / sigma
        print(f"lane fraction rate={rate} seed={seed} epoch={epoch} lane={e} z={z:+.2f}")
        assert abs(z) <= SIGMAS, (e, z)


@pytest.mark.parametrize("rate,seed,epoch", CASES)
def test_no_correlation_along_a_row(rate, seed, epoch):
    k = _stream(rate, seed, epoch)
    for lag in LAGS:
        z = _corr(k[:-lag], k[lag:]) * math.sqrt(k.size - lag)
        print(f"lag rate={rate} seed={seed} epoch={epoch} lag={lag} z={z:+.2f}")
        assert abs(z) <= SIGMAS, (lag, z)


@pytest.mark.parametrize("seed_a,seed_b", SEED_PAIRS)
def test_no_correlation_between_consecutive_seeds(seed_a, seed_b):
    for rate, epoch in ((0.1, 0), (0.5, 2)):
        z = _corr(_stream(rate, seed_a, epoch, N_PAIR), _stream(rate, seed_b, epoch, N_PAIR)) * math.sqrt(N_PAIR)
        print(f"seeds rate={rate} epoch={epoch} {seed_a} / {seed_b} z={z:+.2f}")
        assert abs(z) <= SIGMAS, (rate, z)


@pytest.mark.parametrize("epoch_a,epoch_b", EPOCH_PAIRS)
def test_no_correlation_between_consecutive_epochs(epoch_a, epoch_b):
    for rate, seed in ((0.1, STACK + 1), (0.2, 0)):
        z = _corr(_stream(rate, seed, epoch_a, N_PAIR), _stream(rate, seed, epoch_b, N_PAIR)) * math.sqrt(N_PAIR)
        print(f"epochs rate={rate} seed={seed} {epoch_a} / {epoch_b} z={z:+.2f}")
        assert abs(z) <= SIGMAS, (rate, z)


def test_seed_and_epoch_do_not_trade_places():
    for rate in (0.1, 0.5):
        z = _corr(_stream(rate, 5, 1, N_PAIR), _stream(rate, 6, 0, N_PAIR)) * math.sqrt(N_PAIR)
        print(f"(seed 5, epoch 1) / (seed 6, epoch 0) rate={rate} z={z:+.2f}")
        assert abs(z) <= SIGMAS, (rate, z)


def exact_lane_correlation(threshold: int, distance: int) -> float:
    """corr(K_a, K_a+distance) for a uniform 32-bit word, exactly.  distance 1: both read D[a+1] D[a+2] =: (x, y); given them K_a hangs
    on D[a] and K_a+1 on D[a+3].  distance 2: both read D[a] =: u and D[a+2] =: v; K_a hangs on D[a+1], K_a+2 on D[a+3]."""
    x, y = np.divmod(np.arange(1 << 16, dtype=np.int64), 256)
    free = np.arange(256, dtype=np.int64).reshape(-1, 1)
    if distance == 1:
        ca = np.count_nonzero((free << 16 | x << 8 | y) >= threshold, axis=0)   # over D[a]
        cb = np.count_nonzero((x << 16 | y << 8 | free) >= threshold, axis=0)   # over D[a+3]
    else:
        ca = np.count_nonzero((x << 16 | free << 8 | y) >= threshold, axis=0)   # over D[a+1], (u, v) = (x, y)
        cb = np.count_nonzero((y << 16 | free << 8 | x) >= threshold, axis=0)   # over D[a+3]
    total = 1 << 32
    # counts out of 2^32 words: n_ab = sum ca cb (2^16 pairs of given bytes, 2^8 x 2^8 free), n_a = 2^8 sum ca
    n_ab, n_a, n_b = int((ca * cb).sum()), int(ca.sum()) << 8, int(cb.sum()) << 8
    assert n_a == n_b == ((1 << 24) - threshold) << 8
    return (total * n_ab - n_a * n_b) / math.sqrt(n_a * (total - n_a) * n_b * (total - n_b))


LANE_PAIRS = [(0, 1), (1, 2), (2, 3), (0, 3), (0, 2), (1, 3)]


@pytest.mark.parametrize("rate,seed,epoch", CASES)
def test_lane_pairs_inside_a_group(rate, seed, epoch):
    """the designed dependence, bounded (module docstring)"""
    lanes = _stream(rate, seed, epoch).reshape(-1, 4)
    pairs = lanes.shape[0]
    sigma = 1 / math.sqrt(pairs)
    allowance = 0.0 if rate in INDEPENDENT_RATES else 2.0 ** -8 + 2.0 ** -15
    assert SIGMAS * sigma < 2.0 ** -8, "the sample must be large enough for the bound to bite"
    exact = {d: exact_lane_correlation(ref.threshold(rate), d) for d in (1, 2)}
    for d in (1, 2):
        assert abs(exact[d]) <= allowance, (d, exact[d])
    for a, b in LANE_PAIRS:
        d = 1 if (b - a) % 4 in (1, 3) else 2
        r = _corr(lanes[:, a], lanes[:, b])
        print(f"lanes rate={rate} seed={seed} epoch={epoch} pair={a}{b} r={r:+.5f} z={r / sigma:+.2f} exact={exact[d]:+.5f} "
              f"z about exact={(r - exact[d]) / sigma:+.2f}")
        assert abs(r) <= allowance + SIGMAS * sigma, (a, b, r)
        assert abs(r - exact[d]) <= SIGMAS * sigma, (a, b, r, exact[d])
