"""Schedule of the batched 27 x 27 Jacobi solver (k_jacobi27_quads in k_jacobi27.hip; the tables JSX / JSY / JPLACE / JIDLE_ROW live in
bayes27_jacobi.h, next to the device functions that use them): a resolvable 2-(28, 4, 1) design -- 63 blocks of 4 on
28 points, every pair of points in exactly one block, the blocks split into 9 parallel classes of 7 -- so that one sweep is 9 "super-rounds"
in each of which the 28 slots are 7 quads (4 neighbouring lanes) and all 6 pairs of a quad are rotated before the rows move again.

Construction (found by search, checked below): points = Z_3^3 + one point at infinity (the zero padding slot 27);
blocks = {inf} + cosets of H = <(0,0,1)>, and the translates of B1 = {000, 010, 100, 111}, B2 = {000, 012, 121, 220}; the class C_0 =
{inf + H} + {B1 + (1,1,0) + h, B2 + (0,1,0) + h : h in H}, the classes C_t = C_0 + t for the 9 cosets t of H.  The cosets are walked
x, x, y, x, x, y, x, x, y (x = (1,0,0), y = (0,1,0)): after 9 steps every slot is back where it started.

Prints the two lane permutations (slot s moves to sigma[s]) as C arrays and re-checks them by simulation."""
import itertools

mods = (3, 3, 3)
G = list(itertools.product(range(3), repeat=3))
add = lambda x, y: tuple((a + b) % 3 for a, b in zip(x, y))
sub = lambda x, y: tuple((a - b) % 3 for a, b in zip(x, y))
INF = "inf"
H = [(0, 0, 0), (0, 0, 1), (0, 0, 2)]
B1 = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 1)]
B2 = [(0, 0, 0), (0, 1, 2), (1, 2, 1), (2, 2, 0)]
A1, A2 = (1, 1, 0), (0, 1, 0)


def tr(block, t):
    return frozenset(p if p == INF else add(p, t) for p in block)


C0 = [frozenset([INF] + H)] + [tr(tr(B1, A1), h) for h in H] + [tr(tr(B2, A2), h) for h in H]
assert len(set().union(*C0)) == 28 and sum(len(b) for b in C0) == 28, "C_0 is a partition"
reps = [(i, j, 0) for i in range(3) for j in range(3)]
classes = {t: [tr(b, t) for b in C0] for t in reps}
blocks = set().union(*[set(c) for c in classes.values()])
assert len(blocks) == 63
pairs = {}
for b in blocks:
    for p in itertools.combinations(sorted(b, key=str), 2):
        pairs[p] = pairs.get(p, 0) + 1
assert len(pairs) == 28 * 27 // 2 and set(pairs.values()) == {1}, "every pair exactly once"

# lanes: the blocks of C_0 in quads of 4 neighbouring lanes, the block with the point at infinity last and infinity in lane 27.  Which block
# goes to which quad, and the order inside a quad, are free: ORDER / INNER below were picked (random search + backtracking) so that an
# LDS placement of the rows exists with neither the loads (lane l reads row l) nor the stores (lane l writes row sigma[l]) of ds_*_b128
# ever conflicting: see PLACE at the end.
ORDER = [2, 5, 0, 3, 4, 1]
INNER = [[2, 0, 1, 3], [1, 2, 0, 3], [1, 2, 3, 0], [1, 3, 0, 2], [3, 2, 0, 1], [1, 0, 2, 3], [0, 2, 1]]
pos0 = {}
for q, b in enumerate([C0[1:][i] for i in ORDER] + [C0[0]]):
    pts = sorted([p for p in b if p != INF])
    pts = [pts[i] for i in INNER[q][:3]] + [INF] if INF in b else [pts[i] for i in INNER[q]]
    for m, p in enumerate(pts):
        pos0[p] = 4 * q + m
assert pos0[INF] == 27
inv0 = {v: k for k, v in pos0.items()}


def sigma(delta):
    """lane l -> lane of the same point one class later: pos_{t+delta}(x) = pos_0(x - delta)"""
    s = []
    for l in range(28):
        x = inv0[l]
        s.append(pos0[x] if x == INF else pos0[sub(x, delta)])
    return s


SX, SY = sigma((1, 0, 0)), sigma((0, 1, 0))
assert SX[27] == 27 and SY[27] == 27
# simulation: slots 0..27 at lanes 0..27, nine super-rounds; all pairs of the quads must be all pairs of slots, once each
lane_of = list(range(28))  # lane_of[slot]
met = set()
for step in range(9):
    at = {lane_of[s]: s for s in range(28)}
    for q in range(7):
        quad = [at[4 * q + m] for m in range(4)]
        for a, b in itertools.combinations(quad, 2):
            key = (min(a, b), max(a, b))
            assert key not in met
            met.add(key)
    sg = SY if step % 3 == 2 else SX
    lane_of = [sg[l] for l in lane_of]
assert len(met) == 378 and lane_of == list(range(28)), "one sweep: every pair once, everybody home"
# LDS placement of row r of a matrix, in floats (rows are 28 floats = 7 units of 16 bytes).  gfx950: ds_read_b128 serves the lane groups
# {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} of a half against 64 banks, ds_write_b128 groups of 8 consecutive lanes against 32 banks
# (MI355X_MICROARCH.md, LDS): the start units of a group's rows must differ mod 16 (loads) / mod 8 (stores).
UNIT = {18: 0, 3: 7, 23: 14, 7: 21, 8: 28, 13: 35, 9: 42, 0: 49, 24: 56, 1: 63, 10: 70, 2: 77, 15: 84, 4: 91, 6: 98, 25: 105, 26: 112, 16: 119,
        19: 127, 22: 134, 5: 141, 12: 149, 20: 156, 17: 163, 27: 170, 11: 177, 14: 187, 21: 194}
used = sorted((u, u + 7) for u in UNIT.values())
assert all(a[1] <= b[0] for a, b in zip(used, used[1:])), "rows do not overlap"
LOAD_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19]]
for grp in LOAD_GROUPS:
    assert len({UNIT[r] % 16 for r in grp}) == len(grp)
for sg in (SX, SY):
    for g0 in range(0, 28, 8):
        rows = [sg[l] for l in range(g0, min(28, g0 + 8))]
        assert len({UNIT[r] % 8 for r in rows}) == len(rows)
# the idle lanes 28..31 of a half read a row too: one whose banks the second load group leaves free
free = [r for r in range(28) if UNIT[r] % 16 not in {UNIT[q] % 16 for q in LOAD_GROUPS[1]}]
print("constexpr int JSX[28] = { %s };" % ", ".join(map(str, SX)))
print("constexpr int JSY[28] = { %s };" % ", ".join(map(str, SY)))
print("constexpr int JPLACE[28] = { %s };   // floats; %d floats per matrix" % (", ".join(str(4 * UNIT[r]) for r in range(28)), 4 * used[-1][1]))
print("constexpr int JIDLE_ROW = %d;" % free[0])
