"""NumPy reference of the motion fields of a sequence (bcd_hip_compose_motion, bcd_hip_sequence_push_frame_motion; DESIGN.md section 16, "Sequences with
motion").  TEST INFRASTRUCTURE.

A field is (H, W, 2) float32, (dx, dy) per pixel, in the convention of tests/motion_ref.py.  compose(a, b): a is the field frame t -> u, b the field u -> v in
frame-u pixel order, the result the field t -> v.  Pixel p = (l, c) is BROKEN when a(p) is not finite or |.| >= 2^24, when q = (l + rint(dy1), c + rint(dx1))
lies outside the image, when b(q) is not finite or |.| >= 2^24, or when |rint(dx1) + rint(dx2)| or |rint(dy1) + rint(dy2)| >= 2^24; a broken pixel is
(NaN, NaN), any other the two integer sums as floats.

The step fields of a sequence are a list with one entry per frame: None, or (prev, next) -- the fields frame t -> t - 1 and t -> t + 1, each an array or None
(zero motion).  In a composition one None operand yields the other as it is, two yield None."""
import numpy as np

import motion_ref as mref

F = np.float32
LIMIT = 2 ** 24


def compose(a, b):
    a = np.asarray(a, F)
    H, W = a.shape[:2]
    b = np.asarray(b, F).reshape(H, W, 2)
    ok1, sl, sc = mref.sources(a, H, W)                   # (finite, below 2^24, q inside the image; the indices of the others are 0)
    with np.errstate(invalid="ignore"):
        r1 = np.rint(np.where(ok1[..., None], a, F(0))).astype(np.int64)
        b2 = b[sl, sc]
        ok2 = np.isfinite(b2).all(-1) & (np.abs(b2) < F(LIMIT)).all(-1)
        r2 = np.rint(np.where(ok2[..., None], b2, F(0))).astype(np.int64)
    s = r1 + r2
    ok = ok1 & ok2 & (np.abs(s) < LIMIT).all(-1)
    return np.where(ok[..., None], s.astype(F), F(np.nan)).astype(F)


def compose_fields(a, b):
    """compose with the NULL rules: a None operand is zero motion and yields the other operand as it is"""
    if a is None:
        return b
    if b is None:
        return a
    return compose(a, b)


def step(step_fields, f, towards_next):
    e = step_fields[f]
    return None if e is None else e[1 if towards_next else 0]


def direction(step_fields, t, f):
    """the field frame t -> frame f (1 or 2 frames apart), or None"""
    up = f > t
    mid = t + 1 if up else t - 1
    a = step(step_fields, t, up)
    return a if mid == f else compose_fields(a, step(step_fields, mid, up))


def neighbours(t, R, T):
    return [f for f in range(max(0, t - R), min(T - 1, t + R) + 1) if f != t]


def sequence_fields(step_fields, t, R, T):
    """the fields of the neighbours of frame t, in ascending frame order: what the frame call that defines the pop takes as its motion list"""
    return [direction(step_fields, t, f) for f in neighbours(t, R, T)]


def pair_is_transposed(step_fields, t, f):
    """the keep/transpose rule: the cross masks of the pair are computed once and transposed exactly when neither direction has a field"""
    return direction(step_fields, t, f) is None and direction(step_fields, f, t) is None


def counters(step_fields, R, T):
    """-> dict(cross_computed, cross_transposed, neighbours_warped, fields_composed) of a whole sequence of T frames"""
    c = dict(cross_computed=0, cross_transposed=0, neighbours_warped=0, fields_composed=0)
    for t in range(T):
        for f in neighbours(t, R, T):
            up = f > t
            if f < t and pair_is_transposed(step_fields, t, f):
                c["cross_transposed"] += 1
            else:
                c["cross_computed"] += 1
            c["neighbours_warped"] += direction(step_fields, t, f) is not None
            if abs(f - t) == 2:
                c["fields_composed"] += step(step_fields, t, up) is not None and step(step_fields, t + 1 if up else t - 1, up) is not None
    return c
