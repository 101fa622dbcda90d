"""What the tests of onset-aligned HRIRs share (test_hrtf_onsets_cpu.py, test_binaural_onsets.py): numpy float32 restatements of
fs_hrtf_delay and fs_hrtf_split_onsets (include/frequensee.h, "Onsets"), OnsetModel / OnsetMeshModel — test_binaural_render's
Model and test_binaural_interp's MeshModel with the delayed HRIR in the fold — with their float64 side, and the term the delay adds
to the float64 bound."""
import numpy as np

from test_binaural_interp import Blend, MeshModel
from test_binaural_render import Model

F32 = np.float32
U = 2.0 ** -24


def delay32(h, tau, taps=None):
    """fs_hrtf_delay: i = (int)tau; f = tau - (float)i; g = 1.0f - f; hd[k] = g * x(k - i) + f * x(k - i - 1), x = h inside
    0 .. H-1 and 0.0f outside; fp32, every operation rounded on its own"""
    h = np.asarray(h, np.float32)
    tau = F32(tau)
    H, i = h.shape[0], int(tau)
    f = F32(tau - F32(i))
    g = F32(F32(1.0) - f)
    He = H + i + 1 if taps is None else int(taps)
    assert He >= H + i + 1
    xa, xb = np.zeros(He, np.float32), np.zeros(He, np.float32)
    xa[i:i + H] = h
    xb[i + 1:i + 1 + H] = h
    out = g * xa + f * xb
    assert out.dtype == np.float32
    return out


def delay64(h, tau, taps):
    """the same delay in float64: floor, fraction and both products exact to double"""
    h = np.asarray(h, np.float64)
    i = int(np.floor(tau))
    f = float(tau) - i
    xa, xb = np.zeros(taps + 1), np.zeros(taps + 1)
    xa[i:i + h.shape[0]] = h
    xb[i + 1:i + 1 + h.shape[0]] = h
    return ((1.0 - f) * xa + f * xb)[:taps]


def split32(hrir, threshold, lead):
    """fs_hrtf_split_onsets: per (direction, ear) peak = max |h|, k0 = the lowest k with |h[k]| >= threshold * peak (fp32),
    onset = max(k0 - lead, 0), aligned[k] = h[k + onset] while in range, else 0"""
    h = np.asarray(hrir, np.float32)
    n, _, H = h.shape
    aligned, onsets = np.zeros_like(h), np.zeros((n, 2), np.float32)
    for j in range(n):
        for ear in range(2):
            mag = np.abs(h[j, ear])
            level = F32(threshold) * mag.max()
            assert level.dtype == np.float32
            k0 = int(np.argmax(mag >= level))
            onset = max(k0 - int(lead), 0)
            aligned[j, ear, :H - onset] = h[j, ear, onset:]
            onsets[j, ear] = onset
    return aligned, onsets


class DelayedSet:
    """hrir[q, ear] of a set with onsets in force: the aligned HRIR of q — an index, or with a mesh (t, b, b64, werr) and the
    blend — delayed by q's own onset, He taps in fp32.  As float64 (Blend.astype) it is the float64 side: the exact blend, delayed
    by the onsets' exact blend, in double."""

    def __init__(self, inner, onsets, tri=None):
        self.inner, self.tri = inner, tri
        self.o = np.asarray(onsets, np.float32)
        self.h = getattr(inner, "h", inner)   # the aligned set itself (blend_bound reads it)
        self.omax = F32(self.o.max())
        self.H = self.h.shape[2]
        self.He = self.H + int(self.omax) + 1
        self.shape = self.h.shape[:2] + (self.He,)

    def tau(self, q, ear):
        """(tau in fp32 by the rule, tau of the float64 side, the bound on the fp32 blend's forward error)"""
        if self.tri is None:
            return self.o[q, ear], float(self.o[q, ear]), 0.0
        t, b, b64, werr = q
        o = [self.o[v, ear] for v in self.tri[t]]
        tau = F32(F32(F32(b[0] * o[0]) + F32(b[1] * o[1])) + F32(b[2] * o[2]))
        if tau > self.omax:
            tau = self.omax
        exact = min(sum(float(b64[i]) * float(o[i]) for i in range(3)), float(self.omax))
        return tau, exact, float(sum(werr[i] * float(o[i]) for i in range(3)))

    def __getitem__(self, key):
        q, ear = key
        aligned = self.inner[q, ear]
        tau, tau64, _ = self.tau(q, ear)
        out = delay32(np.asarray(aligned), tau, self.He).view(Blend)
        out.exact = delay64(aligned.astype(np.float64), tau64, self.He)
        return out


class _WithOnsets:
    def set_onsets(self, onsets):
        """fs_hrtf_set_onsets: every held slot is free, the history stays; None clears them"""
        inner = self.hrir.inner if isinstance(self.hrir, DelayedSet) else self.hrir
        if onsets is None:
            self.hrir, self.H = inner, inner.shape[2]
        else:
            self.hrir = DelayedSet(inner, onsets, getattr(self, "tri", None))
            self.H = self.hrir.He
        self.slots = [None] * self.V


class OnsetModel(_WithOnsets, Model):
    """Model (nearest mode) with onsets in force"""

    def __init__(self, table, dirs, hrir, onsets, frame, voices, **kw):
        Model.__init__(self, table, dirs, hrir, frame, voices, **kw)
        self.set_onsets(onsets)


class OnsetMeshModel(_WithOnsets, MeshModel):
    """MeshModel with onsets in force: the blend of the aligned HRIRs, delayed by the blend of the corners' onsets"""

    def __init__(self, table, dirs, hrir, tri, rows, onsets, frame, voices, **kw):
        MeshModel.__init__(self, table, dirs, hrir, tri, rows, frame, voices, **kw)
        self.set_onsets(onsets)


def onset_bound(m, entries, peak=1.0):
    """What onsets add to bound64 (taken with He taps) for the callback m.process(entries) is about to run — blend_bound's
    argument: the folded table is linear in the HRIR, so an HRIR off by dh[k] moves the output by at most max|x| times the voice's
    weight times (sum_k |dh[k]|) (sum_t |f[t]|).  Per end and ear sum_k |dh[k]| is at most the sum of
      the blend's term   sum_i werr_i sum_k |h_i[k]| (1 + u)^3 (with a mesh; weight_error of test_binaural_interp: the two taps a
                         delayed tap reads carry it with weights g + f = 1, the rule's three roundings on top),
      the delay's own    ((1 + u)^3 - 1 + u) sum_k |hA[k]|: f = tau - (float)i is exact (i <= tau < i + 1 <= 2 i, or i = 0),
                         g = 1.0f - f rounds once (at most u, on a factor of |x(k - i)|), and g * x, f * x and their sum round once
                         each on terms whose magnitudes sum to (g + f) sum |hA| = sum |hA|,
      the onset's term   |tau - tau*| sum_j |x(j) - x(j - 1)|, j from 0 to H, x = 0 outside (the total variation): hd[k] = X(k - tau)
                         with X the piecewise linear interpolant of x, so |hd[k] - hd*[k]| is at most the integral of |X'| over the
                         interval between k - tau and k - tau*; those intervals, one per k and |tau - tau*| < 1 long, are disjoint,
                         and on the segment between j - 1 and j, |X'| = |x(j) - x(j - 1)|, of which the intervals cover at most
                         |tau - tau*| in all.  The clamp at omax, applied on both sides, does not widen the difference;
                         |tau - tau*| <= sum_i werr_i o_i, weight_error applied to the onsets' blend (0 in nearest mode).
    Summed over the voices with the larger of the two ends and ears, as bound64's weights are."""
    plan, _ = m.match(entries)
    k64 = np.abs(m.k.astype(np.float64))
    hs = m.hrir
    total = shares = 0.0
    for p in plan:
        if p is None:
            continue
        kind, d0, g0, w0, q0, d1, g1, w1, q1, key = p
        worst = 0.0
        for q, g in ((q0, g0), (q1, g1)):
            f_sum = (np.abs(g.astype(np.float64)) @ k64).sum()
            for ear in range(2):
                aligned = np.abs(np.asarray(hs.inner[q, ear]).astype(np.float64))
                blend = 0.0
                if hs.tri is not None:
                    blend = sum(q[3][i] * np.abs(hs.h[v, ear].astype(np.float64)).sum() for i, v in enumerate(hs.tri[q[0]])) * (1.0 + U) ** 3
                own = ((1.0 + U) ** 3 - 1.0 + U) * (aligned.sum() + blend)
                variation = np.abs(np.diff(np.concatenate([[0.0], hs.inner[q, ear].astype(np.float64), [0.0]]))).sum()
                dtau = hs.tau(q, ear)[2]
                assert dtau < 1.0
                onset = dtau * variation
                worst = max(worst, (blend + own + onset) * f_sum)
        total += float(max(abs(w0), abs(w1))) * worst
    return peak * total
