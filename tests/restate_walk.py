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

Three modes have no line of the reference behind them: the build owns them, and their definition is the prose of
include/frequensee.h (the comments of FS_FLAG_ALL_CONNECTIONS, FS_FLAG_MIS_BALANCE, FS_FLAG_MATERIAL_LOBES) and of DESIGN.md
section 8 (rows "f3" and "f4 (lobes in the walk)").  The model's part for them is written from that prose, again not from
oracle/fs_oracle.c or the kernels, and shares with the build exactly this and nothing else:

  lobes in the walk   the table made at commit from the float32 arrays (Refl = 1 - alpha, tau clamped to Refl + tau <= 1, gains
                      diffuse Refl sigma, specular Refl (1 - sigma), transmitted tau; probability = band mean of a gain / the sum
                      of the three means, diffuse 1 when that sum is 0); word 3 of the bounce's block 0 picks the lobe at a
                      vertex reached by a hit on a material, intervals in the order diffuse, specular, transmitted; specular = the
                      arriving direction mirrored at the stored normal, transmitted = the arriving direction continued from
                      pos - 2 offset n; probability x lobe probability (specular, transmitted: roulette x lobe probability);
                      EvaluatePath takes the gain of the lobe a vertex was LEFT by (diffuse over pi), the diffuse gain over pi at
                      both connection vertices
  all prefixes        every (i, j) of a pair is the candidate path F0..Fi, Bj..B0 with the weight 1 / N(i + j),
                      N(t) = #{(i', j') in [0, D]^2, i' + j' = t}, D = depth (infinite for depth 0), applied to the clamped gain
  balance heuristic   w = p_i / sum_s p_s over s in [max(0, t - D), min(t, D)] with the densities of DESIGN.md section 8, strategy
                      by strategy; the uniform weight instead when a segment has l^2 <= 1e-8 or the ratio is not positive
                      and finite

A contribution (i, j) is flagged iff a decision of turns 0..i-1 of the forward walk, of turns 0..j-1 of the backward walk, its
own connection, a MinSeg or bin-edge test of its path or a weight fallback is fragile: walk() reports fragility per turn.
Whether a deposit of next to no energy is there at all (float32's range ends at 1.2e-38) is one more such decision
(evaluate_candidate).  The frames of these modes carry the bound PER AXIS (Params.axis_bounds, Scene._candidates_by_axis): the
scalar rule above multiplies by 1 / cos at every hit and passes the room's size after 10 ... 14 turns, the per-axis rule follows
the float32 walk's real drift (1e-3 cm after 30 turns) closely enough for walks of 30 ... 40 turns.  The default mode keeps the
scalar rule, and with it its results bit for bit.

What a source's descriptor does (apply_source) and the actors a walk ignores are written from the prose of include/frequensee.h
alone — the comments of fs_source_set_orientation / fs_source_set_directivity, of fs_source_set_object / fs_listener_set_object
and of fs_source_set_order_window — and share with the build exactly this:

  directivity         f = orientation / |orientation| from the float32 values; the emission direction w of a path = the ray with
                      which the source's walk first HIT something (Node.arrive of the first hit-made node among F1..Fi: the
                      model's own float64 ray, nothing is drawn again), without one the unit direction of the connection Fi -> Bj;
                      theta = atan2(|w x f|, w . f), x = theta (K - 1) / pi, k = min(floor x, K - 2), D_b = T[b][k] + (x - k)
                      (T[b][k+1] - T[b][k]) on the float32 table; D_b is the LAST factor of the contribution's energy
  order window        order = the number of the path's nodes that a hit made; outside [lo, hi] nothing is deposited, nothing else
                      changes
  ignored actors      a rectangle has an actor id (Rect.object, Scene.object_ids); the rays of a walk do not see the rectangles of
                      the actor the walk starts from; the connection's query sees every rectangle

D is continuous in w, so it adds no discrete decision and no flag of the kind above; apply_source leaves out the contributions
whose D is too steep for the direction's error (d_flagged, see there).  A frame without table, window and ignored actor is what
it was, bit for bit.
"""
import math
import struct

MASK = 0xFFFFFFFF
NO_MATERIAL = None
NO_OBJECT = None                # a rectangle of no registered actor; a walk that ignores no actor
LOBE_DIFFUSE, LOBE_SPECULAR, LOBE_TRANSMIT = 0, 1, 2


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
        self.lobes = False                   # FS_FLAG_MATERIAL_LOBES: Scene.set_lobes gives the table
        self.axis_bounds = False             # the walk's bound per axis (Scene._candidates_by_axis) instead of the scalar one
        self.bin_size_ms = 1
        self.num_bins = 1000                 # FSAC.h:137
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)


# ---- the world ------------------------------------------------------------------------------------------------------------------------
class Rect:
    """the rectangle {x[axis] = coord, lo[0] <= x[u] <= hi[0], lo[1] <= x[v] <= hi[1]}, u = axis + 1, v = axis + 2 (mod 3)"""
    __slots__ = ("axis", "coord", "u", "v", "ulo", "uhi", "vlo", "vhi", "material", "object")

    def __init__(self, axis, coord, lo, hi, material=NO_MATERIAL, object_id=NO_OBJECT):
        self.axis, self.coord = axis, float(coord)
        self.u, self.v = (axis + 1) % 3, (axis + 2) % 3
        self.ulo, self.vlo = float(lo[0]), float(lo[1])
        self.uhi, self.vhi = float(hi[0]), float(hi[1])
        self.material = material
        self.object = object_id         # the registered actor the rectangle belongs to (fs_scene_set_objects)


# the winding normal e1 x e2 of Scene.triangles' cells is +axis with +0 zeros; a flipped normal has -0 zeros
WINDING = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
FLIPPED = ((-1.0, -0.0, -0.0), (-0.0, -1.0, -0.0), (-0.0, -0.0, -1.0))


class Scene:
    def __init__(self, rects, absorption):
        self.rects = list(rects)
        self.absorption = [list(map(float, row)) for row in absorption]   # [materials][bands]: Absorption[b].Value
        self.bands = len(self.absorption[0])
        self.lobe_gain = self.lobe_prob = None

    def set_lobes(self, transmission, scattering):
        """the lobe table of FS_FLAG_MATERIAL_LOBES from the FLOAT32 values of Absorption / Transmission / Scattering
        [materials][bands]: lobe_gain[m][lobe][b], lobe_prob[m][lobe], lobes in the order diffuse, specular, transmitted"""
        self.lobe_gain, self.lobe_prob = [], []
        for a_row, t_row, s_row in zip(self.absorption, transmission, scattering):
            gains = [[], [], []]
            for a, tau, sigma in zip(a_row, t_row, s_row):
                refl = 1.0 - f32(a)
                tau = min(f32(tau), 1.0 - refl)                          # Refl + tau <= 1
                gains[LOBE_DIFFUSE].append(refl * f32(sigma))
                gains[LOBE_SPECULAR].append(refl * (1.0 - f32(sigma)))
                gains[LOBE_TRANSMIT].append(tau)
            means = [sum(g) / len(g) for g in gains]
            total = sum(means)
            self.lobe_gain.append(gains)
            self.lobe_prob.append([m / total for m in means] if total > 0.0 else [1.0, 0.0, 0.0])

    def pick_lobe(self, material, u):
        """the lobe of the uniform u: [0, P_d) diffuse, [P_d, P_d + P_s) specular, the rest transmitted -> (lobe, its
        probability, fragile: u within 1e-6 of a threshold)"""
        pd, ps, pt = self.lobe_prob[material]
        fragile = abs(u - pd) < 1e-6 or abs(u - (pd + ps)) < 1e-6
        if u < pd:
            return LOBE_DIFFUSE, pd, fragile
        if u < pd + ps:
            return LOBE_SPECULAR, ps, fragile
        return LOBE_TRANSMIT, pt, fragile

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

    def object_ids(self, n=1):
        """the actor id of every triangle of triangles(n), in its order; 0xFFFFFFFF (FS_NO_OBJECT) for a rectangle of no actor"""
        return [0xFFFFFFFF if r.object is NO_OBJECT else r.object for r in self.rects for _ in range(2 * n * n)]

    def _candidates(self, o, d, tmax, e, own=None, e_far=None, far_own=None, ignore=NO_OBJECT):
        """per rectangle the ray's plane meets: (t, rectangle, hit by the model's own arithmetic, robust hit, robust miss, threshold,
        bound at the hit).  e: the bound of the node at o, own: the axis of that node's normal (ACROSS its own wall a node is
        coord +- offset, wrong by float32 rounding only, at most 1e-3 cm at these sizes: the bound is an in-plane matter);
        e_far, far_own: the same for the node the segment ends at (a connection), None for a ray that just ends at tmax;
        ignore: the actor whose rectangles the ray does not see at all (a walk's own actor)"""
        if isinstance(e, tuple):
            return self._candidates_by_axis(o, d, tmax, e, e_far, ignore)
        out = []
        e_all = e + (e_far or 0.0)
        for r in self.rects:
            da = d[r.axis]
            if da == 0.0 or (ignore is not NO_OBJECT and r.object == ignore):
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

    def _candidates_by_axis(self, o, d, tmax, E, E_far, ignore=NO_OBJECT):
        """_candidates with a bound PER AXIS, E = (Ex, Ey, Ez) (Params.axis_bounds).  The scalar rule divides the whole bound by
        |d . n| at every hit, the worst case of every bounce at once, and so passes the room's size after 10 ... 14 turns while
        the float32 walk is still within 1e-3 cm of this one.  To first order a node displaced by delta, its ray's direction
        unchanged (the cone sample depends on the axis-aligned normal alone, the mirrored and the continued direction on the
        arriving one), crosses the plane x[a] = coord displaced by delta_w - (d_w / d_a) delta_a along the in-plane axis w:

            E'_w = E_w + |d_w / d_a| E_a + t 3e-7 / |d_a| + 2e-4,    E'_a = 1e-3

        (3e-7, 2e-4, 1e-3: the direction's error, a coordinate's rounding, the rounding across the node's own wall, as in the
        scalar rule).  Across its own wall a node HAS E_a = 1e-3, so the own-axis exception needs no case of its own.  For a
        connection both ends move: the crossing by at most the sum of what each end alone would move it."""
        out = []
        Ea = tuple(E[i] + E_far[i] for i in range(3)) if E_far is not None else E
        for r in self.rects:
            a, u, v = r.axis, r.u, r.v
            da = d[a]
            if da == 0.0 or (ignore is not NO_OBJECT and r.object == ignore):
                continue
            t = (r.coord - o[a]) / da
            pu, pv = o[u] + t * d[u], o[v] + t * d[v]
            mu, mv = min(pu - r.ulo, r.uhi - pu), min(pv - r.vlo, r.vhi - pv)
            s0 = o[a] - r.coord
            s1 = s0 + tmax * da
            e1 = E[a] if E_far is None else E_far[a]
            clear = abs(s0) > 4.0 * E[a] + 1e-3 and abs(s1) > 4.0 * (e1 + tmax * 3e-7) + 1e-3
            along = abs(t) * 3e-7 / abs(da)
            eu = Ea[u] + abs(d[u] / da) * Ea[a] + along
            ev = Ea[v] + abs(d[v] / da) * Ea[a] + along
            tu, tv = 4.0 * eu + 1e-3, 4.0 * ev + 1e-3
            thr = max(tu, tv, 4.0 * (Ea[a] / abs(da) + along) + 1e-3)      # (of t: where along the ray the plane is met)
            bound = [0.0, 0.0, 0.0]
            bound[a], bound[u], bound[v] = 1e-3, eu + 2e-4, ev + 2e-4
            out.append((t, r, min(mu, mv) >= 0.0 and 0.0 < t <= tmax, clear and s0 * s1 < 0.0 and mu > tu and mv > tv,
                        (clear and s0 * s1 > 0.0) or mu < -tu or mv < -tv, thr, tuple(bound)))
        return out

    def closest(self, o, d, tmax, e=0.0, own=None, ignore=NO_OBJECT):
        """the closest hit: smallest t in (0, tmax] whose in-plane point lies inside the extent -> (rectangle or None, t,
        fragile, bound at the hit).  Fragile: a rectangle that is neither a robust hit nor a robust miss lies no farther than
        the first robust hit, or two robust hits are closer than the threshold.  ignore: the actor of the walk the ray belongs
        to, whose rectangles it passes; any_hit, the connection's query, has no such argument: it ignores nothing."""
        best = None
        robust = []
        cands = self._candidates(o, d, tmax, e, own, ignore=ignore)
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
    """arrive: the direction of the ray whose HIT made the node (None for an end point and for the duplicate node a miss
    pushes); lobe: the lobe the walk left the node by, picked: whether it picked one (lobe mode)"""
    __slots__ = ("pos", "normal", "material", "prob", "bound", "arrive", "lobe", "picked")

    def __init__(self, pos, normal, material, prob, bound=0.0, arrive=None):
        self.pos, self.normal, self.material, self.prob, self.bound = pos, normal, material, prob, bound
        self.arrive, self.lobe, self.picked = arrive, LOBE_DIFFUSE, False


def scalar_bound(bound):
    """a node's bound as one number: itself, or the sum of the per-axis bounds (no less than their norm)"""
    return bound[0] + bound[1] + bound[2] if isinstance(bound, tuple) else bound


def own_axis(node):
    """the axis of the wall the node sits on (its normal is +- that axis), None for an end point"""
    return None if node.normal is None else max(range(3), key=lambda i: abs(node.normal[i]))


def step(scene, prm, pair, side, k, node, ignore=NO_OBJECT):
    """one turn of the loop BEHIND the push of `node` as node k (ARTS.cpp:300-353): None when the roulette ends the walk, else
    (the state the next turn pushes, fragile, hit).  On a miss the state is kept and only the probability changes."""
    words = draw(prm.seed, pair, side, k, 0)
    if prm.russian_roulette and not (u01(words[0]) < prm.rr_prob):       # :301-302, :349-353
        return None
    if prm.lobes and node.arrive is not None and node.material is not NO_MATERIAL:
        return _lobe_step(scene, prm, words, node, ignore)       # (an end point, a vertex without material and the duplicate node do not pick)
    if node.normal is None:                                              # CurrentNormal.IsNearlyZero() :306
        d, fragile = sample_sphere(prm.seed, pair, side, k, words)
        prob = prm.rr_prob / (4.0 * math.pi)                             # :309-310
    else:
        d, cos_theta = sample_cone(node.normal, u01(words[1]), u01(words[2]), prm.cosine)
        fragile = False
        prob = prm.rr_prob * cos_theta / math.pi                         # :316-317
    return _trace(scene, prm, node, node.pos, d, prob, fragile, ignore)


def _trace(scene, prm, node, origin, d, prob, fragile, ignore=NO_OBJECT):
    rect, t, fr, bound = scene.closest(origin, d, prm.max_trace_dist, node.bound, own_axis(node), ignore)   # :340-342, :322-327
    fragile = fragile or fr
    if rect is None:
        return Node(node.pos, node.normal, node.material, prob, node.bound), fragile, False
    n = FLIPPED[rect.axis] if d[rect.axis] > 0.0 else WINDING[rect.axis]  # ImpactNormal faces the side the ray came from
    pos = tuple(origin[i] + t * d[i] + prm.surface_offset * n[i] for i in range(3))   # :345
    return Node(pos, n, rect.material, prob, bound, arrive=d), fragile, True   # :346-347


def _lobe_step(scene, prm, words, node, ignore=NO_OBJECT):
    """the turn behind a vertex that a hit on a material made, in lobe mode: word 3 (the cone sample leaves it unused) picks
    the lobe the walk leaves `node` by, and the node keeps it for EvaluatePath"""
    node.lobe, lobe_prob, fragile = scene.pick_lobe(node.material, u01(words[3]))
    node.picked = True
    n, a, origin = node.normal, node.arrive, node.pos
    if node.lobe == LOBE_DIFFUSE:
        d, cos_theta = sample_cone(n, u01(words[1]), u01(words[2]), prm.cosine)
        prob = prm.rr_prob * cos_theta / math.pi * lobe_prob
    else:
        prob = prm.rr_prob * lobe_prob
        if node.lobe == LOBE_SPECULAR:
            dn = a[0] * n[0] + a[1] * n[1] + a[2] * n[2]
            d = tuple(a[i] - 2.0 * dn * n[i] for i in range(3))
        else:
            # the far side of the surface, 0.1 cm BEYOND the node's own wall.  The own-axis rule of Scene._candidates holds as it
            # stands: across that wall the origin is coord - offset where the node was coord + offset, still the wall's
            # coordinate and a constant, wrong by float32 rounding only, and 0.1 cm clears the 5e-3 cm the rule asks for; in the
            # wall's plane the origin is the node, with the node's bound
            d = a
            origin = tuple(node.pos[i] - 2.0 * prm.surface_offset * n[i] for i in range(3))
    return _trace(scene, prm, node, origin, d, prob, fragile, ignore)


def walk(scene, prm, pair, side, start, turns=None, ignore=NO_OBJECT):
    """ARTS.cpp:279-355 -> (nodes, fragile).  Node k is pushed with the probability the PREVIOUS turn computed (:297), before
    the cap and the roulette; a turn that misses pushes the same place again.  turns: a list that receives, per turn k (the
    one that makes node k + 1), whether a decision of it was fragile.  ignore: the actor the walk starts from (fs_source_set_object
    for side 0, fs_listener_set_object for side 1): every ray of THIS walk passes its rectangles (AddIgnoredActor, :322-327)."""
    node = Node(tuple(float(x) for x in start), None, NO_MATERIAL, 1.0, (0.0, 0.0, 0.0) if prm.axis_bounds else 0.0)  # :287-291
    nodes, fragile, k = [], False, 0
    cap = prm.depth if prm.depth > 0 else (None if prm.russian_roulette and prm.rr_prob < 1.0 else 64)
    while True:
        nodes.append(node)                                               # :297-298
        if cap is not None and k >= cap:
            break
        nxt = step(scene, prm, pair, side, k, node, ignore)
        if nxt is None:
            break
        node, fr, _ = nxt
        fragile = fragile or fr
        if turns is not None:
            turns.append(fr)
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
        return True, abs(tmax) < 1e-3 + 4.0 * (scalar_bound(f.bound) + scalar_bound(b.bound))
    d = (diff[0] / length, diff[1] / length, diff[2] / length)
    hit, fragile = scene.any_hit(f.pos, d, tmax, f.bound, own_axis(f), b.bound, own_axis(b))
    return not hit, fragile


# ---- EvaluatePath, the bin rule ----------------------------------------------------------------------------------------------------------
def evaluate_path_bands_f64(positions, reflectivity, has_material, probability, prm=None, over_pi=None):
    """ARTS.cpp:358-420 for one path and B bands: positions [n][3] (cm), per node its Absorption[b].Value row [B], whether it
    has a geometry component with a material, and its Probability -> (DelaySeconds, [Gain per band], a segment within 1e-5 of MinSeg).
    over_pi (lobe mode): per node whether its row is divided by pi (a diffuse gain) or taken as it is (specular, transmitted)"""
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
            if over_pi is not None and has_material[i] and not over_pi[i]:
                bsdf = reflectivity[i][b]
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


# ---- the build-owned modes: lobe gains along a path, all prefixes, their weights -------------------------------------------------------------
def evaluate_candidate(scene, prm, fwd, bwd):
    """EvaluatePath of the candidate path fwd[0] .. fwd[-1], bwd[-1] .. bwd[0] -> (DelaySeconds, [Gain per band], near MinSeg).
    In lobe mode a vertex contributes the gain of the lobe the walk left it by, the two connection vertices fwd[-1] and bwd[-1]
    the diffuse gain (they were not left along the path: a delta lobe cannot be connected)."""
    path = list(fwd) + list(bwd)[::-1]
    ci = len(fwd) - 1
    refl, over_pi = [], []
    for idx, n in enumerate(path):
        if n.material is NO_MATERIAL:
            refl.append(None)
            over_pi.append(True)
        elif prm.lobes:
            lobe = LOBE_DIFFUSE if idx in (ci, ci + 1) else n.lobe
            refl.append(scene.lobe_gain[n.material][lobe])
            over_pi.append(lobe == LOBE_DIFFUSE)
        else:
            refl.append(scene.absorption[n.material])
            over_pi.append(True)
    delay, gains, near = evaluate_path_bands_f64([n.pos for n in path], refl, [x is not None for x in refl], [n.prob for n in path], prm,
                                                 over_pi)
    # whether a deposit is there at all is a discrete decision too: the build multiplies the factors in float32, whose normal
    # range ends at 1.2e-38, so the energy of a path of some 40 segments is inexact or zero there.  1e-36 leaves a factor of 100
    # for the division by Probability^0.1 (at most some 2 per segment) that follows a segment's smallest intermediate product
    tiny = any(0.0 < g < 1e-36 * prm.energy_gain for g in gains)
    return delay, gains, near or tiny


def strategy_range(t, depth):
    """the strategies s = i of a path with t = i + j surface vertices that a depth cap D leaves: [max(0, t - D), min(t, D)];
    D is infinite for depth 0"""
    return (0, t) if depth <= 0 else (max(0, t - depth), min(t, depth))


def strategies(t, depth):
    """N(t) = #{(i', j') in [0, D]^2, i' + j' = t}"""
    lo, hi = strategy_range(t, depth)
    return hi - lo + 1


COSINE_FLOOR = 1e-6      # an own cosine below it makes the strategy's density next to nothing: next to the `ratio` fallback


def balance_weight(path, s, depth):
    """The balance heuristic of DESIGN.md section 8 for the connected path y_0 (source), y_1 .. y_t (surface vertices with their
    stored normals), y_{t+1} (listener), produced by strategy s (y_1 .. y_s from the source, the rest from the listener), written
    out strategy by strategy -> (weight, fallback, fragile); fallback: None, "segment" (a segment with l^2 <= 1e-8) or "ratio" (the
    ratio not positive or not finite): the uniform weight 1 / N(t) then.

      d_k = unit(y_{k+1} - y_k), L_k = |y_{k+1} - y_k|
      pf_k = Pf(k) |n_{k+1} . d_k| / L_k^2,  Pf(0) = 1 / 4 pi,     Pf(k) = max(0, n_k . d_k) / pi
      pb_k = Pb(k + 1) |n_k . d_k| / L_k^2,  Pb(t + 1) = 1 / 4 pi, Pb(k) = max(0, -n_k . d_{k-1}) / pi
      p_s = prod_{k < s} pf_k  prod_{k > s} pb_k,    w = p_i / sum_{s in [lo, hi]} p_s

    Fragile: a segment that is not exactly of length 0 (the duplicate node is a copy) but shorter than 1e-3 cm + 4 x its nodes'
    bounds, an own density (p_s of the strategy s itself) that a cosine of |c| < COSINE_FLOOR makes next to nothing, or one below
    1e-280 (see there).  A cosine of 0 in ANOTHER strategy's density (a connection along a wall: both nodes have the wall's
    coordinate +- offset) is no decision: max(0, c) is continuous, that strategy just has no density."""
    t = len(path) - 2
    lo, hi = strategy_range(t, depth)
    uniform = 1.0 / (hi - lo + 1)
    seg, fragile = [], False
    for k in range(t + 1):
        diff = [path[k + 1].pos[i] - path[k].pos[i] for i in range(3)]
        l2 = diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2]
        if l2 != 0.0 and math.sqrt(l2) < 1e-3 + 4.0 * (scalar_bound(path[k].bound) + scalar_bound(path[k + 1].bound)):
            fragile = True
        if not l2 > 1e-8:
            return uniform, "segment", fragile
        length = math.sqrt(l2)
        seg.append(((diff[0] / length, diff[1] / length, diff[2] / length), l2))

    def cos(k, j):      # n_k . d_j, 0 for an end point (never asked for in a product that is used)
        n = path[k].normal
        return 0.0 if n is None else n[0] * seg[j][0][0] + n[1] * seg[j][0][1] + n[2] * seg[j][0][2]

    def pf(k):
        P = 1.0 / (4.0 * math.pi) if k == 0 else max(0.0, cos(k, k)) / math.pi
        return P * abs(cos(k + 1, k)) / seg[k][1]

    def pb(k):
        P = 1.0 / (4.0 * math.pi) if k == t else max(0.0, -cos(k + 1, k)) / math.pi
        return P * abs(cos(k, k)) / seg[k][1]

    def p(sp):
        v = 1.0
        for k in range(sp):
            v *= pf(k)
        for k in range(sp + 1, t + 1):
            v *= pb(k)
        return v

    own = [cos(k, k) for k in range(1, s)] + [cos(k + 1, k) for k in range(s)] + \
          [cos(k + 1, k) for k in range(s + 1, t)] + [cos(k, k) for k in range(s + 1, t + 1)]
    fragile = fragile or any(abs(c) < COSINE_FLOOR for c in own)
    total = sum(p(sp) for sp in range(lo, hi + 1))
    # a product of more than some 40 densities (1e-7 each at these sizes) leaves the range of a double, and WHERE it does depends
    # on the order of the multiplications, which the definition shares with no one-pass evaluation: next to the range's end it
    # is a discrete decision with an unknown threshold
    fragile = fragile or not p(s) > 1e-280
    ratio = p(s) / total if total > 0.0 else math.nan
    if not (ratio > 0.0 and math.isfinite(ratio)):
        return uniform, "ratio", fragile
    return ratio, None, fragile


class Contribution:
    __slots__ = ("i", "j", "visible", "fragile", "bin", "energy", "fallback")


class PrefixPair:
    __slots__ = ("fwd", "bwd", "steps", "connections", "contributions", "flagged")


def prefix_pair(scene, prm, idx, src, lis, num_pairs, balance=False, ignore=(NO_OBJECT, NO_OBJECT)):
    """a pair of the all-prefix mode: every (i, j) is the candidate path F0..Fi, Bj..B0 — connect and evaluate as for the end-to-end
    connection, energy = Gain x weight / pairs.  Contribution (i, j) is flagged iff a turn below i of the forward walk, a turn below
    j of the backward walk, its connection, a MinSeg or bin-edge test of its path or a weight fallback is fragile."""
    r = PrefixPair()
    tf, tb = [], []
    r.fwd, _ = walk(scene, prm, idx, 0, src, tf, ignore[0])
    r.bwd, _ = walk(scene, prm, idx, 1, lis, tb, ignore[1])
    r.steps = len(r.fwd) + len(r.bwd) - 2
    r.connections = len(r.fwd) * len(r.bwd)
    r.contributions, r.flagged = [], 0
    ff = [any(tf[:i]) for i in range(len(r.fwd))]
    fb = [any(tb[:j]) for j in range(len(r.bwd))]
    for i in range(len(r.fwd)):
        for j in range(len(r.bwd)):
            c = Contribution()
            c.i, c.j, c.bin, c.energy, c.fallback = i, j, None, None, None
            c.visible, fc = connect(scene, prm, r.fwd[i], r.bwd[j])
            c.fragile = ff[i] or fb[j] or fc
            if c.visible:
                delay, gains, near = evaluate_candidate(scene, prm, r.fwd[:i + 1], r.bwd[:j + 1])
                if balance:
                    w, c.fallback, fw = balance_weight(r.fwd[:i + 1] + r.bwd[j::-1], i, prm.depth)
                else:
                    w, fw = 1.0 / strategies(i + j, prm.depth), False
                c.bin = bin_of(delay, prm.bin_size_ms, prm.num_bins)
                c.energy = [g * w / num_pairs for g in gains]
                c.fragile = c.fragile or near or near_bin_edge(delay, prm.bin_size_ms) or fw
            r.flagged += c.fragile
            r.contributions.append(c)
    return r


class PrefixFrame:
    """what an all-prefix frame deposits, by the model: H [B][bins] summed over the contributions that are not flagged, count =
    their number per bin, flagged = the number of flagged contributions, deposits = the visible ones among the others,
    connections = sum over the pairs of (kf + 1)(km + 1) and steps = the rays of all walks (both exact); what the frame
    exercised: fallbacks by kind, lobes picked by kind, the largest number of prefix combinations of a pair"""

    def __init__(self, scene, prm, src, lis, num_pairs, balance=False, keep_pairs=False, ignore=(NO_OBJECT, NO_OBJECT)):
        self.H = [[0.0] * prm.num_bins for _ in range(scene.bands)]
        self.count = [0] * prm.num_bins
        self.flagged, self.deposits, self.steps, self.connections, self.pairs = 0, 0, 0, 0, []
        self.fallbacks = {"segment": 0, "ratio": 0}
        self.lobes = [0, 0, 0]
        self.most_combinations = self.pairs_over_64 = 0
        for i in range(num_pairs):
            r = prefix_pair(scene, prm, i, src, lis, num_pairs, balance, ignore)
            self.steps += r.steps
            self.connections += r.connections
            self.flagged += r.flagged
            self.most_combinations = max(self.most_combinations, r.connections)
            self.pairs_over_64 += r.connections > 64
            count_lobes(self.lobes, r.fwd + r.bwd)
            if keep_pairs:
                self.pairs.append(r)
            for c in r.contributions:
                if c.fallback:
                    self.fallbacks[c.fallback] += 1
                if c.visible and not c.fragile:
                    self.deposits += 1
                    self.count[c.bin] += 1
                    for b in range(scene.bands):
                        self.H[b][c.bin] += c.energy[b]


def count_lobes(counts, nodes):
    for n in nodes:
        if n.picked:
            counts[n.lobe] += 1


# ---- one pair, one frame -----------------------------------------------------------------------------------------------------------------
class Pair:
    __slots__ = ("fwd", "bwd", "steps", "visible", "fragile", "delay", "bin", "energy")


def pair(scene, prm, i, src, lis, num_pairs, ignore=(NO_OBJECT, NO_OBJECT)):
    """GenerateFullPaths' loop body (ARTS.cpp:217-229) and the pair's deposit (:164-171): the source's walk (side 0), the
    listener's (side 1), the connection of their last nodes, the path F0..Fk, Bm..B0 (:262-267), energy = Gain / pairs"""
    r = Pair()
    r.fwd, ff = walk(scene, prm, i, 0, src, ignore=ignore[0])
    r.bwd, fb = walk(scene, prm, i, 1, lis, ignore=ignore[1])
    r.steps = len(r.fwd) + len(r.bwd) - 2
    r.visible, fc = connect(scene, prm, r.fwd[-1], r.bwd[-1])
    r.fragile = ff or fb or fc
    r.delay, r.bin, r.energy = None, None, None
    if r.visible:
        path = r.fwd + r.bwd[::-1]                                                      # :262-267
        if prm.lobes:
            r.delay, gains, near = evaluate_candidate(scene, prm, r.fwd, r.bwd)
        else:
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

    def __init__(self, scene, prm, src, lis, num_pairs, keep_pairs=False, ignore=(NO_OBJECT, NO_OBJECT)):
        self.H = [[0.0] * prm.num_bins for _ in range(scene.bands)]
        self.count = [0] * prm.num_bins                     # deposits per bin behind H
        self.flagged, self.deposits, self.steps, self.pairs = [], 0, 0, []
        self.connections, self.lobes = num_pairs, [0, 0, 0]      # (lobe mode: the lobes picked, by kind)
        for i in range(num_pairs):
            r = pair(scene, prm, i, src, lis, num_pairs, ignore)
            self.steps += r.steps
            count_lobes(self.lobes, r.fwd + r.bwd)
            if keep_pairs:
                self.pairs.append(r)
            if r.fragile:
                self.flagged.append(i)
            elif r.visible:
                self.deposits += 1
                self.count[r.bin] += 1
                for b in range(scene.bands):
                    self.H[b][r.bin] += r.energy[b]


# ---- what a source's descriptor does to a frame: directivity table, orientation, order window ------------------------------------------------
WALK_RAY_ERROR = 3e-7       # the float32 direction's error of a walk's ray (the figure of the walk's bound)


def emission(fwd, b):
    """the direction a path left the source in: fwd = F0..Fi, the nodes of the source's walk that are on the path, b = the node of
    the listener's walk that Fi is connected to -> (unit direction, its error delta in radians, whether it is the walk's ray).
    The `arrive` of the first node among F1..Fi that a hit made, the exact ray the walk traced; without one (every step so far
    missed: the walk is still at the source) the unit direction of the connection Fi -> Bj, wrong by the two nodes' bounds and a
    coordinate's rounding over its length."""
    for n in fwd[1:]:
        if n.arrive is not None:
            return n.arrive, WALK_RAY_ERROR, True
    f = fwd[-1]
    diff = [b.pos[i] - f.pos[i] for i in range(3)]
    length = math.sqrt(diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2])
    if not length > 0.0:
        return None, math.inf, False
    return (diff[0] / length, diff[1] / length, diff[2] / length), (scalar_bound(f.bound) + scalar_bound(b.bound) + 2e-4) / length, False


def directivity(table, orientation, w):
    """D_b of the emission direction w for the table T[b][k] (K samples, sample k at k pi / (K - 1) from the orientation), in
    float64 on the float32 values the library is given -> ([D_b], [|dD_b / dtheta|] of the interval, k)"""
    f = [f32(x) for x in orientation]
    fl = math.sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2])
    f = [x / fl for x in f]
    cx, cy, cz = w[1] * f[2] - w[2] * f[1], w[2] * f[0] - w[0] * f[2], w[0] * f[1] - w[1] * f[0]
    theta = math.atan2(math.sqrt(cx * cx + cy * cy + cz * cz), w[0] * f[0] + w[1] * f[1] + w[2] * f[2])
    K = len(table[0])
    x = theta * (K - 1) / math.pi
    k = min(int(math.floor(x)), K - 2)
    t = x - k
    D, slope = [], []
    for row in table:
        lo, hi = f32(row[k]), f32(row[k + 1])
        D.append(lo + t * (hi - lo))
        slope.append(abs(hi - lo) * (K - 1) / math.pi)
    return D, slope, k


def order_of(fwd, bwd):
    """the ORDER of the path F0..Fi, Bj..B0: the number of its nodes that a walk step's hit made"""
    return sum(n.arrive is not None for n in fwd) + sum(n.arrive is not None for n in bwd)


class Applied:
    """what a frame deposits for a source with a table, an orientation and an order window, by the model: H, count and deposits
    over the contributions that are not flagged, whose order lies in the window and whose factor D is not fragile; flagged = the
    frame's flagged contributions + d_flagged, the contributions left out for D alone; steps and connections are the frame's
    (the descriptor changes no walk and no visibility query); walk_ray / connection_ray: how many of the deposits took which"""


def apply_source(fr, table=None, orientation=(1.0, 0.0, 0.0), lo=0, hi=None, rtol=0.0, pair_range=None):
    """A frame built with keep_pairs = True under a source descriptor, without walking again (the walks do not depend on it).
    D_b is the last factor of a contribution's energy: after the clamp, the gain, 1 / pairs and the weight.  D is continuous in
    the direction, so it adds no discrete decision, but where it is small and steep its relative error is large: a
    contribution is left out (d_flagged) when |T[b][k+1] - T[b][k]| (K - 1) / pi x delta exceeds rtol / 4 x D_b in some band,
    delta the direction's error (emission), rtol the tolerance the frame is judged with.  pair_range = (begin, end): those pairs
    of the frame alone (flagged, steps and connections are then theirs)."""
    assert fr.pairs, "the frame was built without keep_pairs"
    a = Applied()
    B, bins = len(fr.H), len(fr.H[0])
    a.H = [[0.0] * bins for _ in range(B)]
    a.count = [0] * bins
    a.deposits = a.d_flagged = a.walk_ray = a.connection_ray = a.flagged = a.steps = a.connections = 0
    for r in fr.pairs if pair_range is None else fr.pairs[pair_range[0]:pair_range[1]]:
        a.steps += r.steps
        if isinstance(r, PrefixPair):
            a.connections += r.connections
            items = [(r.fwd[:c.i + 1], r.bwd[:c.j + 1], c.visible, c.fragile, c.bin, c.energy) for c in r.contributions]
        else:
            a.connections += 1
            items = [(r.fwd, r.bwd, r.visible, r.fragile, r.bin, r.energy)]
        for fwd, bwd, visible, fragile, b, energy in items:
            a.flagged += bool(fragile)
            if not visible or fragile or not lo <= order_of(fwd, bwd) <= (math.inf if hi is None else hi):
                continue
            if table is not None:
                w, delta, walked = emission(fwd, bwd[-1])
                if w is None:
                    a.d_flagged += 1
                    continue
                D, slope, _ = directivity(table, orientation, w)
                if any(s * delta > 0.25 * rtol * d for s, d in zip(slope, D)):
                    a.d_flagged += 1
                    continue
                energy = [e * d for e, d in zip(energy, D)]
                a.walk_ray += walked
                a.connection_ray += not walked
            a.deposits += 1
            a.count[b] += 1
            for k in range(B):
                a.H[k][b] += energy[k]
    a.flagged += a.d_flagged
    return a


# ---- the test scene ------------------------------------------------------------------------------------------------------------------------
SOURCE =(700.0, 600.0, 300.0)
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

