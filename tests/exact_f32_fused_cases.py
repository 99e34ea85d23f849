"""Exact-arithmetic cases for the fused fp32 network kernels (csrc/mlp_f32_fused*.hip) on the host emulator: the Case objects of
tests/exact_f32_network_cases.py -- its generate(), restate(), audit() and audit_passes() apply unchanged -- over every shape class of the
fused kernels.  Helper, not a test.

  * CROSS    hidden width 16 / 32 / 64 x every input width 16 .. 128 x every padded output width 16 .. 64, two hidden layers, n = 256: the
             input layer's k-loop from one to eight blocks of 16, the output loop and the first backward product from one to four, every
             2 x 2 tile block of the weight-gradient kernel with and without a ragged half (widths 16, 48, 80, 112) and with inactive waves.
  * TILES    per width one and three hidden layers (no hidden matrix; two) at n = 768: three sample tiles over two slabs and two persistent
             workgroups of the emulator's build (shares of two and one); at width 64 also n = 1280: five tiles over four slabs (three
             one-tile slices, then a two-tile one).  Inputs 48 / 128, padded outputs 16 / 48.
  * LINEAR   one case without a hidden activation.
OUT lies 0, 2 or 3 below the padded width: the trimmed inference then meets whole 16-byte stores, partly masked ones and (stride not a
multiple of four floats) the scalar stores.

Magnitudes.  A sum must stay below 2^24 units of its lattice (C1) while enough results need more than fp16's 11 bits (C3), and both grow
with depth and width: one hidden layer takes the finest values, three the coarsest; the recipes below were chosen per (width, depth) so
that every case passes the unchanged audit, which tests/test_emu_f32_fused.py asserts case by case."""
import exact_f32_network_cases as F

E = F.E
Case = F.Case

ONE = dict(hidden=(E._k(16), 1.0), out=E._k(128), dy=E._k(64))
TWO_NARROW = dict(hidden=(E._k(8), 1.0), out=E._k(32), dy=E._k(16))
TWO_WIDE = dict(hidden=((0.125, 0.25, 0.5), 0.5), out=E._k(16), dy=E._k(8))
THREE_NARROW = dict(hidden=((0.125, 0.25, 0.5), 0.5), out=E._k(8), dy=E._k(4))
THREE_WIDE = dict(hidden=((0.25, 0.5), 0.5), out=E._k(8), dy=E._k(4))


def recipe(W, H):
    if H == 1:
        return ONE
    if H == 2:
        return TWO_WIDE if W == 64 else TWO_NARROW
    return THREE_NARROW if W == 16 else THREE_WIDE


def make(IN, W, OUTP, H, n, act="ReLU"):
    OUT = OUTP - (0, 2, 3)[(IN // 16 + W // 16 + H) % 3]
    name = f"f32f-{IN}-{W}x{H}-{OUTP}" + ("-linear" if act == "None" else "")
    magnitudes = TWO_WIDE if act == "None" else recipe(W, H)  # (nothing is clipped to zero on the way: the sums of a linear network grow faster)
    return Case(name, IN, W, OUT, H, act=act, otype="CutlassMLP", seed=1000 + IN + 3 * W + 7 * OUTP + 11 * H, **magnitudes).at(n)


WIDTHS = (16, 32, 64)
CROSS = [make(IN, W, OUTP, 2, 256) for W in WIDTHS for IN in range(16, 129, 16) for OUTP in (16, 32, 48, 64)]
# (n = 1280 at width 64 only: on the emulator a case costs in proportion to its batch, and the five-tile split does not depend on the width)
TILES = [make(IN, W, OUTP, H, n) for W in WIDTHS for H in (1, 3) for n in (768, 1280) for IN in (48, 128) for OUTP in (16, 48) if n == 768 or W == 64]
LINEAR = [make(80, 32, 48, 2, 256, act="None")]
CASES = CROSS + TILES + LINEAR
