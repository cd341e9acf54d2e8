"""The mixed-radix lengths of the L1FFT loss, without a GPU:

  - util.l1fft_supported against the rule stated here by factoring: L = m 2^k, m odd, m <= 31,
    k >= 3, L <= 1024;
  - the identity csrc/fft_loss.hip rests on, restated in numpy in fp64: with L = m P, P = 2^k,
    n = P n1 + n2 and bin k = k1 + m k2, the m-point DFTs over n1 (stride P), the twiddle
    exp(-2 pi i n2 k1 / L) and the radix-2 DIF stages inside every block of P rows leave bin k at
    row pos(k) = (k mod m) P + brev_P(k div m); the transposed inverse (DIT stages per block,
    conjugate twiddles, unnormalised inverse m-point DFT) returns the input times L.
"""
import numpy as np
import pytest

LENGTHS = [24, 40, 248, 352, 704, 992]


def rule(L: int) -> bool:
    if L < 8 or L > 1024:
        return False
    k = 0
    while L % 2 == 0:
        L //= 2
        k += 1
    return k >= 3 and L <= 31  # L is now the odd part


def split(L: int):
    m = L
    while m % 2 == 0:
        m //= 2
    return m, L // m


def brev(v: int, bits: int) -> int:
    r = 0
    for _ in range(bits):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


def pos(k: int, m: int, P: int) -> int:
    return (k % m) * P + brev(k // m, P.bit_length() - 1)


def radix2_stages(a, L, P, inverse):
    """the butterflies of fft_run over all L rows: half-sizes P/2 .. 1 (DIF) or 1 .. P/2 (DIT),
    butterfly j < L/2 at rows r0, r0 + hs with r0 = (j div hs) 2 hs + (j mod hs)"""
    a = a.copy()
    logP = P.bit_length() - 1
    j = np.arange(L // 2)
    for st in range(logP):
        lm = st if inverse else logP - 1 - st
        hs = 1 << lm
        i = j & (hs - 1)
        r0 = ((j >> lm) << (lm + 1)) + i
        w = np.exp(-2j * np.pi * i / (2 * hs))
        p, q = a[r0], a[r0 + hs]
        if not inverse:
            a[r0], a[r0 + hs] = p + q, (p - q) * w
        else:
            b = q * np.conj(w)
            a[r0], a[r0 + hs] = p + b, p - b
    return a


def odd_forward(x, m, P):
    """m-point DFT over n1 of the rows n1 P + n2, times exp(-2 pi i n2 k1 / L), to row k1 P + n2"""
    L = m * P
    n1 = np.arange(m)
    dft = np.exp(-2j * np.pi * np.outer(n1, n1) / m)            # [k1, n1]
    y = dft @ x.reshape(m, P)                                    # [k1, n2]
    return (y * np.exp(-2j * np.pi * np.outer(n1, np.arange(P)) / L)).reshape(L)


def odd_inverse(y, m, P):
    L = m * P
    k1 = np.arange(m)
    y = y.reshape(m, P) * np.exp(2j * np.pi * np.outer(k1, np.arange(P)) / L)
    return (np.exp(2j * np.pi * np.outer(k1, k1) / m) @ y).reshape(L)  # [n1, n2]


@pytest.mark.parametrize("L", LENGTHS)
def test_split_places_bin_k_at_pos(L):
    m, P = split(L)
    assert m * P == L and m % 2 == 1 and P & (P - 1) == 0 and rule(L)
    rng = np.random.default_rng(L)
    x = rng.standard_normal(L) + 1j * rng.standard_normal(L)
    rows = radix2_stages(odd_forward(x, m, P), L, P, inverse=False)
    where = np.array([pos(k, m, P) for k in range(L)])
    assert sorted(where) == list(range(L))  # pos is a permutation of the rows
    X = np.fft.fft(x)
    assert np.abs(rows[where] - X).max() <= 1e-12 * np.abs(X).max()
    # a formula with k1 and k2 swapped does not pass
    wrong = np.array([(k // P) * P + brev(k % P, P.bit_length() - 1) for k in range(L)])
    assert np.abs(rows[wrong] - X).max() > 1e-3 * np.abs(X).max()


@pytest.mark.parametrize("L", LENGTHS)
def test_transposed_inverse_returns_L_times_input(L):
    m, P = split(L)
    rng = np.random.default_rng(L + 1)
    x = rng.standard_normal(L) + 1j * rng.standard_normal(L)
    rows = radix2_stages(odd_forward(x, m, P), L, P, inverse=False)
    back = odd_inverse(radix2_stages(rows, L, P, inverse=True), m, P)
    assert np.abs(back - L * x).max() <= 1e-12 * L * np.abs(x).max()
    # and from a spectrum placed by pos alone
    X = np.fft.fft(x)
    placed = np.zeros(L, complex)
    for k in range(L):
        placed[pos(k, m, P)] = X[k]
    back = odd_inverse(radix2_stages(placed, L, P, inverse=True), m, P)
    assert np.abs(back - L * x).max() <= 1e-12 * L * np.abs(x).max()


def test_power_of_two_is_the_split_with_m_1():
    for L in (8, 64, 1024):
        m, P = split(L)
        assert (m, P) == (1, L)
        assert [pos(k, m, P) for k in range(L)] == [brev(k, P.bit_length() - 1) for k in range(L)]


def test_rule_examples():
    ok = [8, 16, 24, 40, 96, 160, 224, 248, 320, 352, 384, 480, 704, 992, 1024]
    bad = [0, 4, 12, 20, 25, 264, 296, 1032, 2048, 7, 9, 31, 1023]
    assert all(rule(v) for v in ok) and not any(rule(v) for v in bad)
    assert all(rule(32 * j) for j in range(1, 33))  # every multiple of 32 up to 1024


@pytest.mark.parametrize("other", [8, 704])
def test_l1fft_supported_is_the_rule(other):
    from image_denoising_amd import util

    assert rule(other)
    for L in range(1, 1101):
        assert util.l1fft_supported(L, other) == rule(L), L
        assert util.l1fft_supported(other, L) == rule(L), L
    assert not util.l1fft_supported(0, other) and not util.l1fft_supported(-8, other)
