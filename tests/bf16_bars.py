"""Helpers shared by the bfloat16 parity tests on the host emulator (tests/test_emu_bf16.py) and on the GPU (tests/bf16_cases.py):
plain numpy over the oracle, nothing here touches the emulator or the GPU library.

u = 2^-9 is the unit the bars are written in.  bfloat16 has 8 significant bits: ONE rounding to nearest moves a value by up to
2^-8 of its magnitude = 2 u.  The bucketed backward's fixed-point rule (grid_backward_plan.h, OwnerScale): a record v enters a slice's
sum as round(v * 2^k), k = 30 - ceil(log2(8 * share)) clamped to 20..40, share = (level's sum over the samples of
min(record magnitude of the sample, 4096)) / (slices x chunks of the level); at most half a unit 2^-k is lost per record."""
import math

import numpy as np

from oracle import oracle as O

U = 2.0 ** -9
ONE_ROUNDING = 2 * U * (1 + 2.0 ** -15)  # int -> fp32 (2^-24 of the value) then fp32 -> bfloat16 (2^-8 of it)
TINY = 2.0 ** -133       # bfloat16's smallest subnormal: absolute rounding error of results below 2^-126


def absf(h):
    return O.f2h(np.abs(O.h2f(h)))


def record_counts(og, pos):
    """N_e: records per table entry (every corner of every sample is one record; Nearest: one corner)."""
    idx = O.grid_indices(og, pos)  # [n, L, 2^D] entry index within the level
    F = og.n_features_per_level
    counts = np.zeros(og.n_params, dtype=np.float64)
    for l in range(og.n_levels):
        corners = idx[:, l, :1] if og.interpolation == O.INTERP_NEAREST else idx[:, l, :]
        c = np.bincount(corners.ravel().astype(np.int64), minlength=og.offsets[l + 1] - og.offsets[l])
        counts[og.offsets[l] * F:og.offsets[l + 1] * F] = np.repeat(c, F)
    return counts


def owner_k(level_sum, slices):
    """The header comment's rule, restated: k = 30 - ceil(log2(8 * share)), 20..40; an empty level: 40."""
    if level_sum <= 0 or slices == 0:
        return 40
    share = 8.0 * level_sum / slices
    e = math.frexp(share)[1]  # share < 2^e
    return min(40, max(20, 30 - e))


def level_k(per_sample_magnitude_l, owners):
    """k of one level from the samples' magnitudes [n] and the level's number of owners (slices x chunks).  The kernel adds the clamped
    magnitudes in fp32 in another order: a sum next to a binade edge may fall either side, the coarser k of the two is taken."""
    s = float(np.minimum(np.asarray(per_sample_magnitude_l, np.float64), 4096.0).sum())
    return min(owner_k(s * (1 - 2.0 ** -12), owners), owner_k(s * (1 + 2.0 ** -12), owners))


def max_abs_per_level(dy, L, F):
    return np.abs(O.h2f(dy).astype(np.float64)).reshape(dy.shape[0], L, F).max(axis=2)


def spread(og, per_level):
    """one value per level -> one per parameter"""
    F = og.n_features_per_level
    out = np.zeros(og.n_params)
    for l in range(og.n_levels):
        out[og.offsets[l] * F:og.offsets[l + 1] * F] = per_level[l]
    return out


def second_order_magnitudes(og, pos, ddx, dy):
    """Plain float64 restatement of the second-order corner weight, for MAGNITUDES only: term(d, corner) = scale * ddx_d * pos'_d *
    prod_{e != d} w_e(corner), signed + for the right corner along d and - for the left one.  Returns
      absacc [n_params]: per entry and feature, the sum over samples, corners and d of |dy| * |term| (what the entry accumulated, no
        cancellation between the left / right signs -- the oracle run on |ddx| would let them cancel);
      per_sample [n, L]: max_f |dy| * sum over the corners of |sum_d signed term| -- a sample's share of its level's sum (OwnerScale)."""
    n, D = pos.shape
    L, F, C = og.n_levels, og.n_features_per_level, 1 << og.n_dims
    idx = O.grid_indices(og, pos).astype(np.int64)
    ady = np.abs(O.h2f(dy).astype(np.float64))
    absacc = np.zeros(og.n_params)
    per_sample = np.zeros((n, L))
    for l in range(L):
        sc = float(np.float32(og.scale[l]))
        p = (pos.astype(np.float64) * sc + 0.5).astype(np.float32).astype(np.float64)
        fr = p - np.floor(p)
        if og.interpolation == O.INTERP_SMOOTHSTEP:
            w1, dv = fr * fr * (3 - 2 * fr), 6 * fr * (1 - fr)
        else:
            w1, dv = fr, np.ones_like(fr)
        for c in range(C):
            signed, mag = np.zeros(n), np.zeros(n)
            for d in range(D):
                term = sc * ddx[:, d].astype(np.float64) * dv[:, d]
                for e in range(D):
                    if e != d:
                        term = term * (w1[:, e] if (c >> e) & 1 else 1 - w1[:, e])
                signed += term if (c >> d) & 1 else -term
                mag += np.abs(term)
            per_sample[:, l] += np.abs(signed) * ady[:, l * F:(l + 1) * F].max(axis=1)
            for f in range(F):
                np.add.at(absacc, (og.offsets[l] + idx[:, l, c]) * F + f, mag * ady[:, l * F + f])
    return absacc, per_sample
