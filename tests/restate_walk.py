"""An INDEPENDENT float64 model of the walk, the connection, the evaluation and the deposit of one frame — written from the
reference's lines, not from oracle/fs_oracle.c, with which it shares no code (a helper module like tests/tree_check.py:
plain Python, nothing imported from the oracle or from the package):

  GeneratePath                 Private/AudioRayTracingSubsystem.cpp:279-355
  ConnectSubpaths              Private/AudioRayTracingSubsystem.cpp:235-277
  EvaluatePath                 Private/AudioRayTracingSubsystem.cpp:358-420
  UpdateSource (deposit)       Private/AudioRayTracingSubsystem.cpp:162-173
  AddEnergyAtDelay (bin rule)  Public/FrequenSeeAudioComponent.h:87-91

The world is a list of AXIS-ALIGNED RECTANGLES that the model intersects analytically — no tree, no triangle test; the
library and the oracle get the same rectangles cut into triangles (Scene.triangles).  What the build owns and the model
therefore has to share with it, and nothing else: the random stream (Philox4x32-10 with the counter {pair, bounce << 1 |
side, block, 'FS01'}, u = (word >> 8) 2^-24), which word feeds what, and the sampling map's tangent frame (below).

Everything is float64 while the kernels and the oracle compute in float32, so every DISCRETE decision (which rectangle
is hit, visible or blocked, which side of MinSeg, which bin, accepted or rejected cube sample) reports a margin, and the
walk carries a first-order bound e (cm) of the distance between its node and the float32 one:

    e <- (e + t 3e-7) / |d . n| + 2e-4         at every hit

(3e-7: the float32 direction's error, a few ulp of a component near 1; the division: a position error e moves the hit
point by up to e / cos in the hit plane; 2e-4: the rounding of a float32 coordinate of up to 4 096 cm, 1.2e-4 per
operation, for the impact point and the offset).  A decision whose margin is below 4 x the error that bears on it + 1e-3
is FRAGILE: whether a plane cuts the ray's range at all is decided by the distances of the range's two ends from the
plane, wrong by e (across the wall a node sits on: by rounding only, the node is coord +- offset there); whether the
crossing lies inside the rectangle by the in-plane margin, wrong by (e + t 3e-7) / |d . n|.  A pair with a fragile decision
is flagged and the tests leave it out (they bound how many there may be).
"""
import math
import struct

MASK = 0xFFFFFFFF
NO_MATERIAL = None


def f32(x):
    """the float32 nearest to x, as a Python float: the reference's constants are float literals (0.9f, 0.1f, ...)"""
    return struct.unpack("f", struct.pack("f", x))[0]


# ---- the random stream (Salmon et al. 2011) -----------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0 = (k0 + 0x9E3779B9) & MASK
        k1 = (k1 + 0xBB67AE85) & MASK
    return c0, c1, c2, c3


def draw(seed, pair, side, bounce, block):
    return philox4x32_10((pair, ((bounce << 1) | side) & MASK, block, 0x46533031), (seed & MASK, (seed >> 32) & MASK))


def u01(word):
    return (word >> 8) * 2.0 ** -24


# ---- parameters: the constants compiled into the reference -------------------------------------------------------------------------
class Params:
    def __init__(self, bands=1, **kw):
        self.seed = 0x5EED
        self.depth = 0                       # 0: while (true), ARTS.cpp:294
        self.russian_roulette = True
        self.rr_prob = f32(0.9)              # :282
        self.max_trace_dist = 1000000.0      # :284
        self.surface_offset = f32(0.1)       # :345
        self.connect_pullback = f32(0.1)     # :253
        self.dist_divisor = 1000.0           # :373
        self.min_seg = 1.0                   # :375
        self.prob_exponent = f32(0.1)        # :398
        self.energy_clamp = 1.0              # :410
        self.energy_gain = 10.0              # :413
        self.sound_speed = 343.0             # :362
        self.air_absorption = [f32(0.05)] * bands   # :395
        self.cosine = False                  # the build's cosine-weighted map instead of VRandCone(n, 90 deg)
        self.bin_size_ms = 1
        self.num_bins = 1000                 # FSAC.h:137
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)


# ---- the world ------------------------------------------------------------------------------------------------------------------------
class Rect:
    """the rectangle {x[axis] = coord, lo[0] <= x[u] <= hi[0], lo[1] <= x[v] <= hi[1]}, u = axis + 1, v = axis + 2 (mod 3)"""
    __slots__ = ("axis", "coord", "u", "v", "ulo", "uhi", "vlo", "vhi", "material")

    def __init__(self, axis, coord, lo, hi, material=NO_MATERIAL):
        self.axis, self.coord = axis, float(coord)
        self.u, self.v = (axis + 1) % 3, (axis + 2) % 3
        self.ulo, self.vlo = float(lo[0]), float(lo[1])
        self.uhi, self.vhi = float(hi[0]), float(hi[1])
        self.material = material


# the winding normal e1 x e2 of Scene.triangles' cells is +axis with +0 zeros; a flipped normal has -0 zeros
WINDING = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
FLIPPED = ((-1.0, -0.0, -0.0), (-0.0, -1.0, -0.0), (-0.0, -0.0, -1.0))


class Scene:
    def __init__(self, rects, absorption):
        self.rects = list(rects)
        self.absorption = [list(map(float, row)) for row in absorption]   # [materials][bands]: Absorption[b].Value
        self.bands = len(self.absorption[0])

    def triangles(self, n=1):
        """every rectangle as n x n cells of two triangles (v0, v0 + e1, v0 + e2) -> ([T][3][3] coordinates, [T] material ids
        with 0xFFFF for none).  Both triangles of a cell start at its low corner, so every edge vector is non-negative and the
        float32 winding normal e1 x e2 is +axis with +0 in its other components."""
        tris, mats = [], []
        for r in self.rects:
            du, dv = (r.uhi - r.ulo) / n, (r.vhi - r.vlo) / n

            def point(iu, iv):
                p = [0.0, 0.0, 0.0]
                p[r.axis], p[r.u], p[r.v] = r.coord, r.ulo + iu * du, r.vlo + iv * dv
                return p

            for iu in range(n):
                for iv in range(n):
                    p00, p10, p11, p01 = point(iu, iv), point(iu + 1, iv), point(iu + 1, iv + 1), point(iu, iv + 1)
                    tris += [[p00, p10, p11], [p00, p11, p01]]
                    mats += [0xFFFF if r.material is NO_MATERIAL else r.material] * 2
        return tris, mats

    def _candidates(self, o, d, tmax, e, own=None, e_far=None, far_own=None):
        """per rectangle the ray's plane meets: (t, rectangle, hit by the model's own arithmetic, robust hit, robust miss, threshold,
        bound at the hit).  e: the bound of the node at o, own: the axis of that node's normal (ACROSS its own wall a node is
        coord +- offset, wrong by float32 rounding only, at most 1e-3 cm at these sizes: the bound is an in-plane matter);
        e_far, far_own: the same for the node the segment ends at (a connection), None for a ray that just ends at tmax"""
        out = []
        e_all = e + (e_far or 0.0)
        for r in self.rects:
            da = d[r.axis]
            if da == 0.0:
                continue
            t = (r.coord - o[r.axis]) / da
            pu, pv = o[r.u] + t * d[r.u], o[r.v] + t * d[r.v]
            m = min(pu - r.ulo, r.uhi - pu, pv - r.vlo, r.vhi - pv)      # > 0 inside the extent
            # does the plane cut the segment (0, tmax]?  Decided by the two ends' distances from the plane, each wrong by its
            # node's error across the plane (the far end also by the direction's) — however small d[axis] is, a ray that runs
            # beside the plane (both nodes 0.1 cm off the same wall) never gets near it
            s0 = o[r.axis] - r.coord
            s1 = s0 + tmax * da
            e0 = min(e, 1e-3) if r.axis == own else e
            e1 = e if e_far is None else (min(e_far, 1e-3) if r.axis == far_own else e_far)
            clear = abs(s0) > 4.0 * e0 + 1e-3 and abs(s1) > 4.0 * (e1 + tmax * 3e-7) + 1e-3
            # is the crossing inside the extent?  A position error e moves it by e / |d . n| in the plane
            e_hit = (e_all + abs(t) * 3e-7) / abs(da) + 2e-4
            thr = 4.0 * (e_hit - 2e-4) + 1e-3
            out.append((t, r, m >= 0.0 and 0.0 < t <= tmax, clear and s0 * s1 < 0.0 and m > thr,
                        (clear and s0 * s1 > 0.0) or m < -thr, thr, e_hit))
        return out

    def closest(self, o, d, tmax, e=0.0, own=None):
        """the closest hit: smallest t in (0, tmax] whose in-plane point lies inside the extent -> (rectangle or None, t,
        fragile, bound at the hit).  Fragile: a rectangle that is neither a robust hit nor a robust miss lies no farther than
        the first robust hit, or two robust hits are closer than the threshold."""
        best = None
        robust = []
        cands = self._candidates(o, d, tmax, e, own)
        for c in cands:
            if c[2] and (best is None or c[0] < best[0]):
                best = c
            if c[3]:
                robust.append(c[0])
        robust.sort()
        first = robust[0] if robust else math.inf
        fragile = len(robust) > 1 and robust[1] - robust[0] < max(c[5] for c in cands if c[3])
        for c in cands:
            if not c[3] and not c[4] and c[0] <= first + c[5]:
                fragile = True
        if best is None:
            return None, 0.0, fragile, e
        return best[1], best[0], fragile, best[6]

    def any_hit(self, o, d, tmax, e=0.0, own=None, e_far=0.0, far_own=None):
        """is anything hit on (0, tmax] -> (hit, fragile).  A robust hit settles it; without one every undecided rectangle is fragile."""
        cands = self._candidates(o, d, tmax, e, own, e_far, far_own)
        if any(c[3] for c in cands):
            return True, False
        return any(c[2] for c in cands), any(not c[4] for c in cands)


# ---- the sampling maps -----------------------------------------------------------------------------------------------------------------
def sample_sphere(seed, pair, side, bounce, words):
    """FMath::VRand (ARTS.cpp:308): points of the cube [-1, 1)^3 until 1e-4 < |v|^2 <= 1, normalised.  The first point comes
    from words 1-3 of the bounce's block 0 (word 0 was the roulette's), retry i from words 0-2 of block i -> (dir, fragile)"""
    r = words[1:4]
    fragile = False
    for attempt in range(16):
        if attempt:
            r = draw(seed, pair, side, bounce, attempt)[0:3]
        x, y, z = 2.0 * u01(r[0]) - 1.0, 2.0 * u01(r[1]) - 1.0, 2.0 * u01(r[2]) - 1.0
        l2 = x * x + y * y + z * z
        fragile = fragile or abs(l2 - 1.0) < 1e-6 or abs(l2 - 1e-4) < 1e-6
        if 1e-4 < l2 <= 1.0:
            inv = 1.0 / math.sqrt(l2)
            return (x * inv, y * inv, z * inv), fragile
    return (0.0, 0.0, 1.0), fragile


def tangent_frame(n):
    """the orthonormal frame (t, b, n) of Duff et al. 2017 — it reads the SIGN of n.z, also of a zero: for a wall whose
    normal has n.z = 0 the frame depends on whether that zero is +0 (the winding normal) or -0 (the flipped one)"""
    sg = math.copysign(1.0, n[2])
    a = -1.0 / (sg + n[2])
    b = n[0] * n[1] * a
    return (1.0 + sg * n[0] * n[0] * a, sg * b, -sg * n[0]), (b, sg + n[1] * n[1] * a, -n[1])


def sample_cone(n, U, V, cosine):
    """FMath::VRandCone(n, pi / 2) (ARTS.cpp:313): theta = 2 pi U about n, phi = fmod(acos(2 V - 1), pi / 2) from n; or the
    cosine-weighted map sin^2 phi = V -> (dir, cos theta)"""
    if cosine:
        cphi, sphi = math.sqrt(1.0 - V), math.sqrt(V)
    else:
        phi = math.fmod(math.acos(2.0 * V - 1.0), 0.5 * math.pi)
        cphi, sphi = math.cos(phi), math.sin(phi)
    theta = 2.0 * math.pi * U
    lx, ly = sphi * math.cos(theta), sphi * math.sin(theta)
    t, b = tangent_frame(n)
    d = [lx * t[i] + ly * b[i] + cphi * n[i] for i in range(3)]
    inv = 1.0 / math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])      # GetSafeNormal
    d = (d[0] * inv, d[1] * inv, d[2] * inv)
    return d, d[0] * n[0] + d[1] * n[1] + d[2] * n[2]                   # :315


# ---- GeneratePath ----------------------------------------------------------------------------------------------------------------------
class Node:
    __slots__ = ("pos", "normal", "material", "prob", "bound")

    def __init__(self, pos, normal, material, prob, bound=0.0):
        self.pos, self.normal, self.material, self.prob, self.bound = pos, normal, material, prob, bound


def own_axis(node):
    """the axis of the wall the node sits on (its normal is +- that axis), None for an end point"""
    return None if node.normal is None else max(range(3), key=lambda i: abs(node.normal[i]))


def step(scene, prm, pair, side, k, node):
    """one turn of the loop BEHIND the push of `node` as node k (ARTS.cpp:300-353): None when the roulette ends the walk, else
    (the state the next turn pushes, fragile, hit).  On a miss the state is kept and only the probability changes."""
    words = draw(prm.seed, pair, side, k, 0)
    if prm.russian_roulette and not (u01(words[0]) < prm.rr_prob):       # :301-302, :349-353
        return None
    if node.normal is None:                                              # CurrentNormal.IsNearlyZero() :306
        d, fragile = sample_sphere(prm.seed, pair, side, k, words)
        prob = prm.rr_prob / (4.0 * math.pi)                             # :309-310
    else:
        d, cos_theta = sample_cone(node.normal, u01(words[1]), u01(words[2]), prm.cosine)
        fragile = False
        prob = prm.rr_prob * cos_theta / math.pi                         # :316-317
    rect, t, fr, bound = scene.closest(node.pos, d, prm.max_trace_dist, node.bound, own_axis(node))   # :340-342
    fragile = fragile or fr
    if rect is None:
        return Node(node.pos, node.normal, node.material, prob, node.bound), fragile, False
    n = FLIPPED[rect.axis] if d[rect.axis] > 0.0 else WINDING[rect.axis]  # ImpactNormal faces the side the ray came from
    pos = tuple(node.pos[i] + t * d[i] + prm.surface_offset * n[i] for i in range(3))   # :345
    return Node(pos, n, rect.material, prob, bound), fragile, True        # :346-347


def walk(scene, prm, pair, side, start):
    """ARTS.cpp:279-355 -> (nodes, fragile).  Node k is pushed with the probability the PREVIOUS turn computed (:297), before
    the cap and the roulette; a turn that misses pushes the same place again."""
    node = Node(tuple(float(x) for x in start), None, NO_MATERIAL, 1.0)  # :287-291
    nodes, fragile, k = [], False, 0
    cap = prm.depth if prm.depth > 0 else (None if prm.russian_roulette and prm.rr_prob < 1.0 else 64)
    while True:
        nodes.append(node)                                               # :297-298
        if cap is not None and k >= cap:
            break
        nxt = step(scene, prm, pair, side, k, node)
        if nxt is None:
            break
        node, fr, _ = nxt
        fragile = fragile or fr
        k += 1
    return nodes, fragile


# ---- ConnectSubpaths -------------------------------------------------------------------------------------------------------------------
def connect(scene, prm, f, b):
    """ARTS.cpp:252-254: visible iff nothing is hit from F towards B on (0, |B - F| - pullback] -> (visible, fragile)"""
    diff = [b.pos[i] - f.pos[i] for i in range(3)]
    l2 = diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2]
    if not l2 > 1e-8:                                                    # GetSafeNormal() == 0: a zero-length trace
        return True, False
    length = math.sqrt(l2)
    tmax = length - prm.connect_pullback
    if not tmax > 0.0:
        return True, abs(tmax) < 1e-3 + 4.0 * (f.bound + b.bound)
    d = (diff[0] / length, diff[1] / length, diff[2] / length)
    hit, fragile = scene.any_hit(f.pos, d, tmax, f.bound, own_axis(f), b.bound, own_axis(b))
    return not hit, fragile


# ---- EvaluatePath, the bin rule ----------------------------------------------------------------------------------------------------------
def evaluate_path_bands_f64(positions, reflectivity, has_material, probability, prm=None):
    """ARTS.cpp:358-420 for one path and B bands: positions [n][3] (cm), per node its Absorption[b].Value row [B], whether it
    has a geometry component with a material, and its Probability -> (DelaySeconds, [Gain per band], a segment within 1e-5 of MinSeg)"""
    prm = prm or Params(bands=len(reflectivity[0]))
    B = len(prm.air_absorption)
    energy, scaled, near = [1.0] * B, 0.0, False
    for i in range(len(positions) - 1):                                                 # :368
        node_distance = math.dist(positions[i], positions[i + 1]) / prm.dist_divisor    # :373
        scaled += node_distance                                                         # :374
        near = near or abs(node_distance - prm.min_seg) < 1e-5
        if node_distance < prm.min_seg:                                                 # :375-378
            continue
        geometry = 1.0 / (4.0 * math.pi * node_distance * node_distance)                # :391
        pw = probability[i] ** prm.prob_exponent                                        # :398
        for b in range(B):
            bsdf = reflectivity[i][b] / math.pi if has_material[i] else 1.0             # :382-386
            e = energy[b]
            e *= bsdf                                                                   # :392
            e *= geometry                                                               # :393
            e *= math.exp(-prm.air_absorption[b] * node_distance)                       # :395-397
            e /= pw                                                                     # :398
            energy[b] = e
    gains = [min(e, prm.energy_clamp) * prm.energy_gain for e in energy]                # :410, :413
    return scaled / prm.sound_speed, gains, near                                        # :419


def bin_of(delay_seconds, bin_size_ms=1, num_bins=1000):
    """FSAC.h:89: FMath::Clamp(FMath::FloorToInt((DelaySeconds * 1000.f) / BinSizeMs), 0, EnergyBuffer.Num() - 1)"""
    return int(min(max(math.floor(delay_seconds * 1000.0 / bin_size_ms), 0), num_bins - 1))


def near_bin_edge(delay_seconds, bin_size_ms=1, rel=2e-5):
    x = delay_seconds * 1000.0 / bin_size_ms
    return abs(x - round(x)) < rel * max(abs(x), 1.0)


# ---- one pair, one frame -----------------------------------------------------------------------------------------------------------------
class Pair:
    __slots__ = ("fwd", "bwd", "steps", "visible", "fragile", "delay", "bin", "energy")


def pair(scene, prm, i, src, lis, num_pairs):
    """GenerateFullPaths' loop body (ARTS.cpp:217-229) and the pair's deposit (:164-171): the source's walk (side 0), the
    listener's (side 1), the connection of their last nodes, the path F0..Fk, Bm..B0 (:262-267), energy = Gain / pairs"""
    r = Pair()
    r.fwd, ff = walk(scene, prm, i, 0, src)
    r.bwd, fb = walk(scene, prm, i, 1, lis)
    r.steps = len(r.fwd) + len(r.bwd) - 2
    r.visible, fc = connect(scene, prm, r.fwd[-1], r.bwd[-1])
    r.fragile = ff or fb or fc
    r.delay, r.bin, r.energy = None, None, None
    if r.visible:
        path = r.fwd + r.bwd[::-1]                                                      # :262-267
        refl = [scene.absorption[n.material] if n.material is not NO_MATERIAL else None for n in path]
        r.delay, gains, near = evaluate_path_bands_f64([n.pos for n in path], refl, [x is not None for x in refl],
                                                       [n.prob for n in path], prm)
        r.bin = bin_of(r.delay, prm.bin_size_ms, prm.num_bins)
        r.energy = [g / num_pairs for g in gains]                                       # :164, :170
        r.fragile = r.fragile or near or near_bin_edge(r.delay, prm.bin_size_ms)
    return r


class Frame:
    """what a frame of `num_pairs` pairs deposits, by the model: H [B][bins] summed over the pairs that are not flagged,
    flagged = their indices, deposits = the visible ones among the others, steps = the rays of all walks (exact: the
    roulette is integer arithmetic)"""

    def __init__(self, scene, prm, src, lis, num_pairs, keep_pairs=False):
        self.H = [[0.0] * prm.num_bins for _ in range(scene.bands)]
        self.count = [0] * prm.num_bins                     # deposits per bin behind H
        self.flagged, self.deposits, self.steps, self.pairs = [], 0, 0, []
        for i in range(num_pairs):
            r = pair(scene, prm, i, src, lis, num_pairs)
            self.steps += r.steps
            if keep_pairs:
                self.pairs.append(r)
            if r.fragile:
                self.flagged.append(i)
            elif r.visible:
                self.deposits += 1
                self.count[r.bin] += 1
                for b in range(scene.bands):
                    self.H[b][r.bin] += r.energy[b]


# ---- the test scene ------------------------------------------------------------------------------------------------------------------------
SOURCE = (700.0, 600.0, 300.0)
LISTENER = (2300.0, 1400.0, 500.0)


def make_test_scene():
    """A room of 3000 x 2000 x 800 cm (longer than the 10 m of MinSeg: segments on both sides of it) whose x = 3000 side is
    open (misses), y-walls without a material, and a free-floating slab [1400, 1500] x [300, 1300] x [100, 700] of a second
    material between source and listener (blocked connections).  4 bands, 2 materials."""
    X, Y, Z = (0.0, 3000.0), (0.0, 2000.0), (0.0, 800.0)
    rects = [Rect(0, X[0], (Y[0], Z[0]), (Y[1], Z[1]), 0),
             Rect(1, Y[0], (Z[0], X[0]), (Z[1], X[1]), NO_MATERIAL), Rect(1, Y[1], (Z[0], X[0]), (Z[1], X[1]), NO_MATERIAL),
             Rect(2, Z[0], (X[0], Y[0]), (X[1], Y[1]), 0), Rect(2, Z[1], (X[0], Y[0]), (X[1], Y[1]), 0)]
    sx, sy, sz = (1400.0, 1500.0), (300.0, 1300.0), (100.0, 700.0)
    for c in sx:
        rects.append(Rect(0, c, (sy[0], sz[0]), (sy[1], sz[1]), 1))
    for c in sy:
        rects.append(Rect(1, c, (sz[0], sx[0]), (sz[1], sx[1]), 1))
    for c in sz:
        rects.append(Rect(2, c, (sx[0], sy[0]), (sx[1], sy[1]), 1))
    absorption = [[0.85, 0.7, 0.55, 0.4], [0.3, 0.45, 0.6, 0.75]]
    return Scene(rects, absorption)

