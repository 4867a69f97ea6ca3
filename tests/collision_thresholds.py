"""Collision cases that sit exactly on the thresholds of handleCollisions, and a brute-force numpy restatement of that function.

A pair collides by two strict comparisons on d2 = ((0 + dx*dx) + dy*dy) + dz*dz (nanoflann's term order, d = x_i - x_j):
d2 < 3.0 (RadiusResultSet on the squared distance, src/multirotor_simulator.cpp:326) and d2 < crit(i, j) =
((arm_i + prop_i) + arm_j) + prop_j (:342-346).  For a threshold T the generator returns pairs of four classes, found by scaling a
random direction to |d| = sqrt(T) and stepping one coordinate of one UAV by -3 ... +3 ulps:
  at      d2 == T as written, and >= T however the sum is contracted        -> must NOT qualify
  below   d2 == nextafter(T, 0), and < T however the sum is contracted      -> must qualify
  fma-in  d2 <  T as written, but d2 >= T contracted -> qualifies; an FMA in the sum loses the pair
  fma-out d2 >= T as written, but d2 <  T contracted -> does not qualify; an FMA gains it
"contracted" is what a compiler makes of the sum under -ffp-contract=fast: fma(dz, dz, fma(dy, dy, dx*dx)) or
fma(dz, dz, fma(dx, dx, dy*dy)) — half the pairs of an fma class have the one on the far side of T, half the other (classify).
d2 is always recomputed from the stored doubles x_i - x_j.  Seeded, pure numpy (fma is emulated exactly with fractions.Fraction), no
GPU, no library code."""
import functools
import math
from fractions import Fraction

import numpy as np

CLASSES = ("at", "below", "fma-in", "fma-out")
PER_CLASS = 16      # pairs per class and threshold among the near-origin and cell-face anchors
NEAR_BUDGET = 20000 # candidates per pair among the near anchors: a few dozen are used, the bound only ends a search gone wrong
FAR_BUDGET = 256    # candidates per pair of the far-out group (|x| = 2^17 m); what they yield is counted, not demanded
FAR_PER_CLASS = 4
PITCH = 31.5        # = 18 * 1.75 = 14 * 2.25: a shift by multiples of it keeps a point on the faces of both cell sizes; pairs are PITCH apart
                    # (anchors reach 7 m from their slot's origin)
HAIR = 2.0 ** -40   # "a hair beside" a face: dyadic, so x_i - x_j stays exact

# airframe constants (arm_length, prop_radius, mass) as config/uavs/*.yaml has them; "giant" is no shipped airframe: its crit of 3.5
# lies above the search radius, which makes d2 < 3.0 itself decide a pair (every shipped crit is below 1.04)
AIRFRAME = {"x500": (0.25, 0.15, 2.0), "f450": (0.225, 0.11, 1.7), "f550": (0.27, 0.11, 2.3), "naki": (0.20, 0.13, 7.5),
            "t650": (0.325, 0.19, 3.5), "giant": (1.0, 0.75, 2.0)}
SQRT3_UP, SKIN = 1.7320508075688775, 0.5
LIST_R2 = (SQRT3_UP + SKIN) * (SQRT3_UP + SKIN) * (1.0 + 1e-9) + 1e-5  # collide_work.h (single GPU)


def crit(a, b):
    """crit(i, j) for airframes a (UAV i) and b (UAV j), in the reference's order"""
    return ((AIRFRAME[a][0] + AIRFRAME[a][1]) + AIRFRAME[b][0]) + AIRFRAME[b][1]


def thresholds(planar=False):
    """[(name, T, airframe of the first UAV, airframe of the second)] — the asymmetric pairs come with both of their values"""
    out = [("3.0", 3.0, "giant", "giant")]
    for a in ("x500", "f550", "naki"):
        out.append((f"crit {a}/{a}", crit(a, a), a, a))
    for a, b in (("f450", "t650"), ("naki", "t650")):
        lo, hi = sorted((crit(a, b), crit(b, a)))
        assert lo < hi
        out.append((f"crit {a}/{b} smaller", lo, a, b))
        out.append((f"crit {a}/{b} larger", hi, a, b))
    if not planar:
        out.append(("LIST_R2", LIST_R2, "x500", "x500"))
    return out


def d2_written(a, b):
    """the squared distance as the reference writes it, on float64 scalars or arrays [..., 3]"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d0, d1, d2 = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return ((0.0 + d0 * d0) + d1 * d1) + d2 * d2


def fma(a, b, c):
    """round(a * b + c) with one rounding"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def d2_contracted(a, b, partial=True):
    """the evaluations a contracting compiler can make of the sum.  With 0 + dx*dx folded to dx*dx, the first addition has a product on
    either side and a compiler fuses one of them: fma(dy, dy, dx*dx) or fma(dx, dx, dy*dy) (LLVM takes the left one); the second
    addition can only become fma(dz, dz, .).  Returns ([the two full contractions], [the three partial ones])."""
    d0, d1, d2 = (float(a[k]) - float(b[k]) for k in range(3))
    p0, p1 = d0 * d0, d1 * d1
    fy, fx = fma(d1, d1, p0), fma(d0, d0, p1)
    if d2 == 0.0:  # (the plane: the second addition adds nothing, fused or not)
        return [fy, fx], [fy, fx, p0 + p1]
    return [fma(d2, d2, fy), fma(d2, d2, fx)], [fy + d2 * d2, fx + d2 * d2, fma(d2, d2, p0 + p1)] if partial else None


def classify(xi, xj, T, form=None):
    """class of the pair at threshold T, or None.  The classes are disjoint: `at` and `below` are pairs on which no contraction, full
    or partial, changes the side of T (they pin < against <= and the term order); the fma classes are pairs that a full contraction
    carries across T — any of the two (form None), or the one that fuses dy*dy (form 0) or dx*dx (form 1) into the first addition.
    In the plane the two hardly ever coincide (the fused product has to lie in the binade of T), so the generators ask for them in turn:
    a contracted kernel gets half the pairs of an fma class wrong whichever product its compiler fuses."""
    d0, d1, d2 = (float(xi[k]) - float(xj[k]) for k in range(3))  # (Python floats are IEEE doubles: the same roundings as numpy's)
    w = ((0.0 + d0 * d0) + d1 * d1) + d2 * d2
    if abs(w - T) > 2 * math.ulp(T):  # (one fused product moves the sum by less than an ulp)
        return None
    full, _ = d2_contracted(xi, xj, partial=False)
    flips = [(f < T) != (w < T) for f in full]
    if any(flips) if form is None else flips[form]:
        return "fma-in" if w < T else "fma-out"
    if any(flips) or any((f < T) != (w < T) for f in d2_contracted(xi, xj)[1]):
        return None
    if w == T:
        return "at"
    if w == math.nextafter(T, 0.0):
        return "below"
    return None


def near_anchors():
    """the origin; points on and a hair beside faces and corners of the 1.75 m and 2.25 m cells, negative ones included (dyadic)"""
    out = [(0.0, 0.0, 0.0)]
    for e in (1.75, 2.25):
        for h in (0.0, -HAIR, HAIR):
            out += [(e + h, 0.5, 0.25), (-e + h, 0.5, 0.25), (0.5, -2 * e + h, 0.25), (0.25, 0.5, 3 * e + h), (e + h, e + h, e + h),
                    (-e + h, -e + h, -e + h), (-e + h, e + h, -2 * e + h), (h, h, h)]
    return out


def far_anchors():
    """|x| = 2^17 m (131 072 m): there x_i - x_j is a multiple of 2^-35, and the pair's cells are 75 000 cells out"""
    return [(2.0 ** 17, 0.5, 0.25), (-2.0 ** 17, -1.75, 2.25), (2.0 ** 17 + 1.75, 2.25, 0.0), (-2.0 ** 17 + 0.25, 0.0, -2.25)]


BATCH = 256


def candidates(rng, xj, T, planar=False, direction=None):
    """BATCH candidate partners of the UAV at xj: directions (direction(rng, BATCH) -> [BATCH, 3], default uniform) scaled to
    |d| = sqrt(T), one coordinate solved again from the stored doubles of the other two, then stepped by 0, -1, +1, ... +3 ulps.
    Yields the x_i whose d2 as written lies within two ulps of T, candidate by candidate, step by step."""
    xj = np.asarray(xj, dtype=np.float64)
    u = rng.normal(size=(BATCH, 3)) if direction is None else np.asarray(direction(rng, BATCH), dtype=np.float64)
    if planar:
        u[:, 2] = 0.0
    u /= np.sqrt((u * u).sum(axis=1))[:, None]
    xi = xj + u * math.sqrt(T)
    if planar:
        xi[:, 2] = xj[2]
    rows = np.arange(BATCH)
    c = rng.integers(2 if planar else 3, size=BATCH)
    # the other coordinates are stored doubles now (beside 2^17 they are multiples of 2^-35): solve for this one again
    d = xi - xj
    sq = d * d
    sq[rows, c] = 0.0
    room = T - sq.sum(axis=1)
    ok = room >= 0.0025  # |d_c| < 0.05: a step of an ulp there moves d2 by much less than an ulp of T
    centre = xj[c] + np.copysign(np.sqrt(np.where(ok, room, 1.0)), d[rows, c])
    steps, lo, hi = [centre], centre, centre
    for _ in range(3):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        steps += [lo, hi]
    close = []
    for v in steps:
        x = xi.copy()
        x[rows, c] = v
        close.append((x, ok & (np.abs(d2_written(x, xj) - T) <= 2 * math.ulp(T))))
    for k in np.nonzero(np.any([m for _, m in close], axis=0))[0]:
        for x, m in close:
            if m[k]:
                yield x[k].copy()


def uniform_dir(axis):
    """directions mostly along x (axis 0) or y (axis 1) in the plane: a full contraction fuses ONE product into the first addition, and
    carries d2 across T either way only where that product lies in the binade of T (classify: form 1 wants dx*dx there, form 0 dy*dy)"""
    def draw(r, n):
        u = np.zeros((n, 3))
        u[:, axis] = r.choice([-1.0, 1.0], n)
        u[:, 1 - axis] = r.uniform(-0.45, 0.45, n)
        return u
    return draw


def find_partner(rng, xj, T, cl, budget=20000, planar=False, direction=None, accept=None, form=None):
    """x_i of class `cl` at threshold T against the UAV at xj (accept(x_i): a further condition; form: see classify), or None when the
    budget of candidates runs out"""
    if planar and direction is None and form is not None:
        direction = uniform_dir(1 - form)
    for _ in range(0, budget, BATCH):
        for xi in candidates(rng, xj, T, planar, direction):
            if classify(xi, xj, T, form) == cl and (accept is None or accept(xi)):
                return xi
    return None


def find_pairs(rng, T, anchors, slots, want, budget, planar):
    """{class: [(x_i, x_j)]} with up to `want` pairs per class; pair k of a class sits at anchors[k % len] shifted into a grid slot of its
    own, and gets `budget` candidates.  The pairs of an fma class fall for the two contractions in turn (classify)."""
    found = {c: [] for c in CLASSES}
    k = 0
    for cl in CLASSES:
        for m in range(want):
            base = np.array(anchors[k % len(anchors)], dtype=np.float64)
            k += 1
            if planar:
                base[2] = 0.0
            xj = base + PITCH * np.array(slots[-1], dtype=np.float64)
            xi = find_partner(rng, xj, T, cl, budget, planar, form=m % 2 if cl.startswith("fma") else None)
            if xi is not None:
                found[cl].append((xi, xj))
                slots.pop()
    return found


def grid_slots(rng, count, planar=False):
    """`count` distinct grid slots, shuffled: integer triples, negative ones included (z >= 0).  planar: z = 0, and neither x nor y is
    0 — no UAV of a planar scenario has a coordinate of exactly zero in the plane (see Cases)"""
    side = int(math.ceil(count ** (1 / (2 if planar else 3)))) + 2
    span = [a - side // 2 for a in range(side)]
    if planar:
        cells = [(a, b, 0) for a in span for b in span if a != 0 and b != 0]
    else:
        cells = [(a, b, c) for a in span for b in span for c in range(side)]
    rng.shuffle(cells)
    cells = cells[:count]
    if not planar and (0, 0, 0) in cells:  # the first pair (the anchors start with the origin) sits at the origin itself
        cells.remove((0, 0, 0))
    return cells + ([] if planar else [(0, 0, 0)])


class Cases:
    """pos[n, 3], airframe[n] (names), and the pair table: first[m], second[m] (UAV indices), thr[m] (index into .thresholds),
    cls[m] (index into CLASSES), far[m].  UAVs are ordered threshold by threshold, all first members of the group's pairs and then all
    second members: airframes come in runs, and the runs end inside 64-UAV blocks.
    planar: the pairs lie in the plane z = 0 with dz = 0, for UAVs that rest on the ground while step kernels evaluate them; the fma
    classes still exist for (0 + dx^2) + dy^2.  There no x or y is exactly 0.0 (the grid leaves the axes out): a FAST step moves a
    resting UAV by some 1e-33 m per tick — rounding residue of its contracted sums — which every other coordinate absorbs without a
    trace and a coordinate of exactly zero does not, and the GPU tests demand positions bit-identical to those set."""

    def __init__(self, seed=20251, planar=False, per_class=PER_CLASS, far_per_class=FAR_PER_CLASS):
        rng = np.random.default_rng(seed)
        self.planar = planar
        self.thresholds = thresholds(planar)
        need = len(self.thresholds) * len(CLASSES) * (per_class + far_per_class) + 8
        slots = grid_slots(rng, need, planar)
        pos, af, first, second, thr, cls, far = [], [], [], [], [], [], []
        self.counts = {}
        for t, (name, T, a, b) in enumerate(self.thresholds):
            near = find_pairs(rng, T, near_anchors(), slots, per_class, NEAR_BUDGET, planar)
            out = find_pairs(rng, T, far_anchors(), slots, far_per_class, FAR_BUDGET, planar)
            group = []
            for ci, c in enumerate(CLASSES):
                self.counts[(name, c)] = (len(near[c]), len(out[c]))
                group += [(p, ci, False) for p in near[c]] + [(p, ci, True) for p in out[c]]
            # an airframe run must not end on a 64-UAV block boundary (the step kernels treat a block of one airframe apart from a mixed
            # one): if a run of this group would, its last far-out pair goes — that group promises no count
            base = len(pos)
            while (base + len(group)) % 64 == 0 or (base + 2 * len(group)) % 64 == 0:
                last = max(q for q, (_, _, isfar) in enumerate(group) if isfar)
                name_c = (name, CLASSES[group[last][1]])
                self.counts[name_c] = (self.counts[name_c][0], self.counts[name_c][1] - 1)
                del group[last]
            m = len(group)
            for k, ((xi, xj), ci, isfar) in enumerate(group):
                first.append(base + k)
                second.append(base + m + k)
                thr.append(t)
                cls.append(ci)
                far.append(isfar)
            for k, ((xi, xj), ci, isfar) in enumerate(group):
                pos.append(xi)
                af.append(a)
            for k, ((xi, xj), ci, isfar) in enumerate(group):
                pos.append(xj)
                af.append(b)
        self.pos = np.array(pos, dtype=np.float64)
        self.airframe = np.array(af, dtype=object)
        self.first, self.second = np.array(first), np.array(second)
        self.thr, self.cls, self.far = np.array(thr), np.array(cls), np.array(far)
        self.n = len(self.pos)

    @classmethod
    def from_table(cls, planar, thresholds_, pos, airframe, first, second, thr, klass):
        c = object.__new__(cls)
        c.planar, c.thresholds, c.counts = planar, thresholds_, {}
        c.pos, c.airframe = np.array(pos, dtype=np.float64), np.array(airframe, dtype=object)
        c.first, c.second, c.thr, c.cls = np.array(first), np.array(second), np.array(thr), np.array(klass)
        c.far, c.n = np.zeros(len(c.first), dtype=bool), len(c.pos)
        return c

    def T(self, k):
        return self.thresholds[self.thr[k]][1]

    def pairs_of(self, name, cl):
        t = [x[0] for x in self.thresholds].index(name)
        return np.nonzero((self.thr == t) & (self.cls == CLASSES.index(cl)))[0]

    def report(self):
        return "\n".join(f"{name:26s} {c:8s} near {a:3d}  far-out {b:2d}" for (name, c), (a, b) in self.counts.items())

    def check_counts(self, per_class=PER_CLASS):
        """the condition of the suite: every class holds `per_class` pairs per threshold among the near anchors, every pair is of its
        class by the stored doubles, and pairs keep 4 m from one another"""
        short = {k: v for k, v in self.counts.items() if v[0] < per_class}
        assert not short, f"classes short of {per_class} pairs: {short}"
        for k in range(len(self.first)):
            assert classify(self.pos[self.first[k]], self.pos[self.second[k]], self.T(k)) == CLASSES[self.cls[k]], k
        partner = np.full(self.n, -1)
        partner[self.first], partner[self.second] = self.second, self.first
        assert (partner >= 0).all()
        for lo in range(0, self.n, 512):
            d = np.sqrt(d2_written(self.pos[lo:lo + 512, None, :], self.pos[None, :, :]))
            rows = np.arange(lo, min(self.n, lo + 512))
            d[rows - lo, rows] = np.inf
            d[rows - lo, partner[rows]] = np.inf
            assert d.min() >= 4.0, f"pairs closer than 4 m to one another: {d.min()}"


@functools.lru_cache(maxsize=None)
def cases(planar=False):
    """the suite's cases (seeded: the same in every process); planar: pairs in the plane z = 0 with dz = 0"""
    return Cases(planar=planar)


def constants(airframe):
    """(arm_length[n], prop_radius[n], mass[n]) of an array of airframe names"""
    c = np.array([AIRFRAME[a] for a in airframe], dtype=np.float64)
    return c[:, 0], c[:, 1], c[:, 2]


def restatement(pos, arm, prop, mass, crash, rebounce=100.0, radius2=3.0):
    """handleCollisions (src/multirotor_simulator.cpp:321-358) by brute force, per UAV:
      neighbours[i] : ascending indices j != i with d2(i, j) < radius2                     (the radius search)
      partners[i]   : those of them with d2 < crit(i, j)                                   (contact, seen from i)
      crashed[n]    : crash mode — UAV j of every contact (i, j) is crashed (:348); all zero in elastic mode
      force[n, 3]   : elastic mode — sum over partners[i], ascending, of ((rebounce * normalized(x_i - x_j)) * m_i) * (m_j / (m_i + m_j))
    positions must be finite"""
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    neighbours, partners = [None] * n, [None] * n
    crashed, force = np.zeros(n, dtype=np.int32), np.zeros((n, 3))
    for lo in range(0, n, 512):
        hi = min(n, lo + 512)
        dd = d2_written(pos[lo:hi, None, :], pos[None, :, :])
        near = dd < radius2
        near[np.arange(hi - lo), np.arange(lo, hi)] = False
        for i in range(lo, hi):
            nb = np.nonzero(near[i - lo])[0]
            neighbours[i] = nb
            keep = []
            for j in nb:
                if dd[i - lo, j] < ((arm[i] + prop[i]) + arm[j]) + prop[j]:
                    keep.append(int(j))
                    if crash:
                        crashed[j] = 1
                    else:
                        r = pos[i] - pos[j]
                        z = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
                        if z > 0:
                            r = r / np.sqrt(z)
                        force[i] += ((rebounce * r) * mass[i]) * (mass[j] / (mass[i] + mass[j]))
            partners[i] = np.array(keep, dtype=np.int64)
    return dict(neighbours=neighbours, partners=partners, crashed=crashed, force=force)


def expected_pair_outcome(cases, k, crash):
    """what the rule says about pair k (UAV a = first, b = second) literally: (a acts on b, b acts on a) with "acts" = d2 < 3.0 and
    d2 < crit(actor, other).  Elastic: the ACTOR is pushed; crash mode: the OTHER is crashed."""
    a, b = cases.first[k], cases.second[k]
    w = float(d2_written(cases.pos[a], cases.pos[b]))
    w2 = float(d2_written(cases.pos[b], cases.pos[a]))
    ab = w < 3.0 and w < crit(cases.airframe[a], cases.airframe[b])
    ba = w2 < 3.0 and w2 < crit(cases.airframe[b], cases.airframe[a])
    return ab, ba


# ---- clusters for the search tick's fallback path ------------------------------------------------------------------------------------
def _apart(x, others, af, afs):
    """no contact either way between a UAV of airframe af at x and the UAVs (position, airframe) of `others`, with some room to spare"""
    return all(float(d2_written(x, y)) > max(crit(af, g), crit(g, af)) + 0.02 for y, g in zip(others, afs))


def _near(axis, spread):
    return lambda r, n: np.asarray(axis) + r.normal(0, spread, (n, 3))


@functools.lru_cache(maxsize=None)
def overflow_clusters(seed=411, clusters=24):
    """(pos, airframe, [cluster]): clusters whose centre UAV has more contacts than the four hits a query keeps, so that the search
    tick's fallback path decides a threshold case.  A cluster is a dict(kind, centre, at, below) of UAV indices (at, below: lists).
      fillers (x500 centre and partners at crit x500/x500; or an f450 centre with t650 partners at the smaller value of their crit):
        six x500 0.3 - 0.6 m from the centre, one partner of class `at`, one of class `below`.  The six stand in the half-space
        opposite the two and touch neither, and the two do not touch each other: the centre is the only UAV that can act on them.
        Sharp in elastic mode (the centre's force); in crash mode the six crash the centre whatever the threshold partners do.
      shell-at, shell-below (an f450 centre inside six t650 near the axes of a rotated octahedron, none touching another): at
        d2 == 0.85 exactly the f450 acts on a t650 (0.85 < 0.8500000000000001) — a hit of the centre in either mode — while the t650
        does not act on the f450 (0.85 < 0.85 is false).  shell-at: all six are such `at` partners — six hits, and in crash mode
        nobody crashes the centre.  shell-below: one of the six is an ulp below 0.85 instead — it alone crashes the centre.
        Sharp in crash mode: the centre's flag is the fallback path's decision on one threshold partner.
    UAV order is shuffled within a cluster."""
    rng = np.random.default_rng(seed)
    slots = grid_slots(rng, clusters)
    pos, af, out = [], [], []
    for k in range(clusters):
        kind = ("fillers", "shell-at", "shell-below")[k % 3]
        a, b = ("x500", "x500") if kind == "fillers" and k % 2 == 0 else ("f450", "t650")
        T = min(crit(a, b), crit(b, a))
        xc = np.array(near_anchors()[k % len(near_anchors())]) + PITCH * np.array(slots[k], dtype=np.float64)
        members, cls = [(xc, a)], ["centre"]
        placed = []
        if kind == "fillers":
            u = rng.normal(size=3)
            u /= np.sqrt(u @ u)
            v = np.cross(u, rng.normal(size=3))
            v /= np.sqrt(v @ v)
            axes = [("at", u), ("below", 0.1 * u + v)]  # some 85 degrees apart: 1.2 m between the two
        else:
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            axes = [("below" if kind == "shell-below" and m == 0 else "at", s * q[:, m // 2]) for m, s in enumerate((1, -1, 1, -1, 1, -1))]
        for cl, axis in axes:
            xi = find_partner(rng, xc, T, cl, direction=_near(axis, 0.08), accept=lambda x: _apart(x, placed, b, [b] * len(placed)))
            assert xi is not None, (k, kind, cl)
            placed.append(xi)
            members.append((xi, b))
            cls.append(cl)
        if kind == "fillers":
            away = -(placed[0] - xc) - (placed[1] - xc)
            away /= np.sqrt(away @ away)
            while len(members) < 9:
                w = away + rng.normal(0, 0.35, 3)
                x = xc + w / np.sqrt(w @ w) * rng.uniform(0.3, 0.6)
                if _apart(x, placed, "x500", [b, b]):
                    members.append((x, "x500"))
                    cls.append("filler")
        order = rng.permutation(len(members))
        base = len(pos)
        where = base + np.argsort(order)  # member m sits at where[m]
        for m in order:
            pos.append(members[m][0])
            af.append(members[m][1])
        out.append(dict(kind=kind, centre=int(where[0]), at=[int(where[m]) for m, c in enumerate(cls) if c == "at"],
                        below=[int(where[m]) for m, c in enumerate(cls) if c == "below"]))
    return np.array(pos), np.array(af, dtype=object), out


# ---- the list radius, with cells and the in-cell quantisation against it -------------------------------------------------------------
WIDE_EDGE_INV = 1.0 / (SQRT3_UP + SKIN + 0.0179491924)  # collide_work.h INV_CELL_WIDE: cells of the list rebuild are floor(x * this)


def wide_cell(x):
    return np.floor(np.asarray(x, dtype=np.float64) * WIDE_EDGE_INV).astype(np.int64)


@functools.lru_cache(maxsize=None)
def list_radius_cases(seed=977):
    """(pos, first[m], second[m], cls[m], direction[m, 3]): pairs at LIST_R2 whose second UAV sits at an in-cell position hostile to a
    1/1024 quantisation of the 2.25 m cell — fractions k/1024 +- 1e-12, 1023.999/1024, and coordinates a hair below zero (cell -1, at
    its far face) — and whose first UAV lies in the neighbour cell of each of the 26 directions.  Per direction: three pairs of class
    `at` and of class `below`, one of each fma class."""
    rng = np.random.default_rng(seed)
    edge = 1.0 / WIDE_EDGE_INV
    dirs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    plan = [("at", 0), ("below", 1), ("at", 2), ("below", 0), ("at", 1), ("below", 2), ("fma-in", 0), ("fma-out", 1)]
    slots = grid_slots(rng, len(dirs) * len(plan))
    pos, first, second, cls, direction = [], [], [], [], []
    row = 0
    for s in dirs:
        s = np.array(s)
        for cl, variant in plan:
            cell = 7 * np.array(slots.pop(), dtype=np.int64)  # 7 cells = 15.75 m between pairs (all of them within one cell of their slot's)
            if variant == 2:  # a row along x beyond the grid: y and z a hair below zero
                cell = np.array([7 * (40 + row), 0, 0], dtype=np.int64)
                row += 1
            for _ in range(400):
                # in-cell fraction per coordinate: towards the face the pair crosses (so that sqrt(LIST_R2) = 2.232 m reaches the
                # neighbour cell), mid-cell where it stays; always on a 1/1024 line, or at the far end of the cell
                k = np.where(s > 0, rng.integers(700, 1024, 3), np.where(s < 0, rng.integers(1, 324, 3), rng.integers(384, 640, 3)))
                frac = k / 1024.0 + rng.choice([-1e-12, 1e-12], 3)
                if variant == 1:
                    frac = np.where(s > 0, 1023.999 / 1024.0, frac)
                xj = (cell + frac) * edge
                if variant == 2:  # a hair below zero: cell -1, and the pair crosses into cell 0 or stays
                    xj[1] = -6.9e-22 if s[1] >= 0 else xj[1]
                    xj[2] = -1e-300 if s[2] >= 0 else xj[2]
                cj = wide_cell(xj)
                xi = find_partner(rng, xj, LIST_R2, cl, budget=BATCH, direction=lambda r, n: s + r.normal(0, 0.25, (n, 3)),
                                  accept=lambda x: np.array_equal(wide_cell(x) - cj, s))
                if xi is not None:
                    break
            assert xi is not None, (tuple(s), cl, variant)
            first.append(len(pos)); pos.append(xi)
            second.append(len(pos)); pos.append(xj)
            cls.append(CLASSES.index(cl)); direction.append(s)
    return np.array(pos), np.array(first), np.array(second), np.array(cls), np.array(direction)


# ---- pairs across a slab boundary (sharded swarms) and pairs deep in a neighbour list (fused evaluation), on the ground plane --------
@functools.lru_cache(maxsize=None)
def straddle_cases(seed=613, per_class=5):
    """planar pairs whose second UAV lies at x < 0 and whose first at x > 0, a column of pairs 8 m apart in y: sorted by x, the lower
    half of the swarm is exactly the second members — in two slabs every partner is foreign to the other.  (The directions are
    mostly along y: a contracted sum differs from the written one by the rounding of one product, which can carry d2 across T either
    way only where that product lies in the binade of T; elsewhere one fma class lives on ties alone and the other is hardly found.)"""
    rng = np.random.default_rng(seed)
    th = thresholds(planar=True)
    pos, af, first, second, thr, klass = [], [], [], [], [], []
    row = 0
    for t, (name, T, a, b) in enumerate(th):
        for ci, cl in enumerate(CLASSES):
            for q in range(per_class):
                xj = np.array([(-0.125, -0.0625, -HAIR, -0.03125)[row % 4], 8.0 * (row // 2 + 1) * (-1) ** row, 0.0])
                towards = ((lambda r, n: np.stack([r.uniform(0.25, 0.45, n), r.choice([-1.0, 1.0], n), np.zeros(n)], axis=1)) if q % 2 == 0 else
                           (lambda r, n: np.stack([np.ones(n), r.uniform(-0.45, 0.45, n), np.zeros(n)], axis=1)))
                xi = find_partner(rng, xj, T, cl, planar=True, direction=towards, accept=lambda x: x[0] > 0, form=q % 2)
                assert xi is not None and xi[0] > 0
                first.append(len(pos)); pos.append(xi); af.append(a)
                second.append(len(pos)); pos.append(xj); af.append(b)
                thr.append(t); klass.append(ci)
                row += 1
    c = Cases.from_table(True, th, pos, af, first, second, thr, klass)
    assert np.all(c.pos[:, :2] != 0.0)
    return c


@functools.lru_cache(maxsize=None)
def deep_list_cases(seed=733):
    """planar clusters of seven: a centre UAV, its threshold partner, and five x500 on a circle of 1.6 m around the centre — inside the
    list radius of the centre, in contact with nobody.  The centre has the highest index, so its list holds the five and the partner,
    the partner as entry 6 (even clusters) or entry 5 (odd ones): behind the entries a fused step launch prefetches."""
    rng = np.random.default_rng(seed)
    th = thresholds(planar=True)
    pos, af, first, second, thr, klass = [], [], [], [], [], []
    k = 0
    for t, (name, T, a, b) in enumerate(th):
        for ci, cl in enumerate(CLASSES):
            for layout in (0, 1):
                xc = np.array([PITCH * (k % 12 + 1), PITCH * (k // 12 + 1), 0.0]) + np.array(near_anchors()[k % 25]) * [1.0, 1.0, 0.0]
                xp = find_partner(rng, xc, T, cl, planar=True, form=layout)
                ang = math.atan2(xp[1] - xc[1], xp[0] - xc[0])
                ring = [xc + 1.6 * np.array([math.cos(ang + math.pi / 3 * m), math.sin(ang + math.pi / 3 * m), 0.0]) for m in range(1, 6)]
                members = [(p, "x500") for p in ring]
                members.insert(5 - layout, (xp, a))
                base = len(pos)
                pos += [m[0] for m in members] + [xc]
                af += [m[1] for m in members] + [b]
                first.append(base + 5 - layout); second.append(base + 6)
                thr.append(t); klass.append(ci)
                k += 1
    c = Cases.from_table(True, th, pos, af, first, second, thr, klass)
    assert np.all(c.pos[:, :2] != 0.0)
    return c
