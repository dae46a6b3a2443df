"""Constructed motion fields for the tests of bcd_hip_compose_motion and of sequences with motion (tests/test_sequence_motion_cpu.py,
tests/test_gpu_compose_motion.py, tests/test_gpu_sequence_motion.py).  TEST INFRASTRUCTURE.

field_pairs(W, H): pairs (a, b) of (H, W, 2) float32 fields to compose -- random vectors with fractional parts, about a third of which leave the image at
the first step and a third of those that stay at the second -- and special_pair(W, H), whose vectors cycle through the values at which the definition
branches: NaN, +-inf, +-2^24 and the floats next to it, -0.0, the halves +-0.5, 1.5, 2.5 (round to even), and second steps whose sum with the first reaches
2^24.

step_fields(kind, W, H, T): the per-step fields of a sequence of T frames, one (prev, next) pair per frame, see its docstring."""
import numpy as np

F = np.float32
BIG = F(2.0 ** 24)
SPECIALS = [F(np.nan), F(np.inf), F(-np.inf), BIG, -BIG, np.nextafter(BIG, F(0)), -np.nextafter(BIG, F(0)), F(-0.0), F(0.0), F(0.5), F(-0.5), F(1.5), F(-1.5),
            F(2.5), F(-2.5), F(1.0), F(-1.0), F(0.49999997), F(3.0)]


def random_field(W, H, seed, reach):
    """vectors uniform in [-reach, reach] with fractional parts (a tenth of them exact halves)"""
    rng = np.random.default_rng(seed)
    f = ((rng.random((H, W, 2)) * 2 - 1) * reach).astype(F)
    halves = rng.random((H, W, 2)) < 0.1
    return np.where(halves, (np.floor(f) + F(0.5)).astype(F), f).astype(F)


def special_field(W, H, shift):
    """every pair (x, y) of SPECIALS in turn, starting `shift` pairs in"""
    n = len(SPECIALS)
    k = (np.arange(W * H) + shift) % (n * n)
    f = np.stack([np.array(SPECIALS, F)[k % n], np.array(SPECIALS, F)[k // n]], -1)
    return f.reshape(H, W, 2).astype(F)


def special_pair(W, H):
    a = special_field(W, H, 0)
    b = special_field(W, H, 7)
    # where the first step stays put or moves by one, second steps that bring a sum to exactly +-2^24 and to one below it
    l, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    edge = (l + c) % 5 == 0
    b[..., 0] = np.where(edge, np.where(c % 2 == 0, np.nextafter(BIG, F(0)), -np.nextafter(BIG, F(0))), b[..., 0])
    return a, b.astype(F)


def field_pairs(W, H):
    reach = max(W, H) * 0.75 + 1
    pairs = [(random_field(W, H, 11, reach), random_field(W, H, 12, reach)), (random_field(W, H, 13, 2.5), random_field(W, H, 14, reach)),
             (random_field(W, H, 15, reach), special_field(W, H, 3)), special_pair(W, H)]
    z = np.zeros((H, W, 2), F)
    return pairs + [(z, special_field(W, H, 5)), (special_field(W, H, 9), z)]


def translation(W, H, dx, dy):
    f = np.empty((H, W, 2), F)
    f[..., 0], f[..., 1] = dx, dy
    return f


PREV = [(4, -2), (-3, 4), (4, 3), (-4, -4), (2, 4)]       # the translations of "moving": frame t -> t - 1 ...
NEXT = [(2, -3), (-4, 4), (3, 4), (4, -4), (-3, 2)]       # ... and t -> t + 1; 2 -> 0 is (1, 7), 2 -> 4 is (7, 0)


def step_fields(kind, W, H, T):
    """-> [(prev, next)] * T, prev = frame t -> t - 1, next = t -> t + 1 (arrays (H, W, 2) or None)
      "null"    every field None
      "zero"    every field zero-valued
      "moving"  integer translations of up to 4 px per step (a vector two frames away exceeds the search radius 6), some with NaN pixels, some with
                sub-pixel values; the `next` field of frame 1 is None and so is frame 3's `prev`
      "partly"  only frame 2 moves: its two fields are translations, every other field is None"""
    if kind == "null":
        return [(None, None)] * T
    if kind == "zero":
        return [(np.zeros((H, W, 2), F), np.zeros((H, W, 2), F)) for _ in range(T)]
    if kind == "partly":
        return [(translation(W, H, 2, -1), translation(W, H, -3, 1)) if t == 2 else (None, None) for t in range(T)]
    assert kind == "moving"
    rng = np.random.default_rng(31)
    out = []
    for t in range(T):
        prev = translation(W, H, *PREV[t % 5])
        nxt = translation(W, H, *NEXT[t % 5])
        if t % 2 == 0:                                      # sub-pixel parts that round back to the translation, and a few halves that do not
            prev = (prev + (rng.random((H, W, 2)).astype(F) - F(0.5)) * F(0.8)).astype(F)
            prev[(rng.random((H, W)) < 0.02)] += F(0.5)
        if t % 2 == 1:
            nxt[(rng.random((H, W)) < 0.03)] = F(np.nan)
            prev[(rng.random((H, W)) < 0.02), 0] = F(np.inf)
        out.append((prev, nxt))
    out[1] = (out[1][0], None)
    out[3] = (None, out[3][1])
    return out
