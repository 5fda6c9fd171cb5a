"""The inputs of tests/test_operator_shapes_gpu.py discriminate (no GPU needed): conditions on tests/shape_cases.py,
checked with the numpy references alone, so that a GPU test cannot pass by not looking.

* On `mixed_flow` every outcome of SPEC §9 (wall fallback, limited, unlimited) and both answers to "does the next lane
  hold my i0+1 samples" cover a share of the cells, for both traces.
* Mutated references: each plausible kernel error below is written into a *copy* of the numpy reference in this file
  (never into the library) and must change at least one bit of the result on at least one case of the table; the test
  prints the cases that catch it."""
import numpy as np
import pytest

import diagnostics_ref as D
import forces_ref as F
import maccormack_ref as M
import oracle_lib as O
import shape_cases as C
from ref_support import row_partials_one_trip, same_bits
from shape_cases import DT

I = (slice(1, -1),) * 3
IDS = [f"N{N}-{C.dname(t)}" for N, t in C.SHAPES]


# ---- the flow takes every branch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dtype", [s for s in C.SHAPES if s[0] >= 13], ids=[i for i, s in zip(IDS, C.SHAPES) if s[0] >= 13])
def test_mixed_flow_takes_every_branch(N, dtype):
    u, v, w = C.mixed_flow(N, dtype, N)
    d0 = C.normal_field(N, dtype, N)
    fallback, limited, unlimited = M.outcomes(d0, u, v, w, DT)
    fwd, rev = M.adjacency(u, v, w, DT)
    print(f"N={N} {C.dname(dtype)}: fallback {fallback:.3f} limited {limited:.3f} unlimited {unlimited:.3f} "
          f"next lane adjacent {fwd:.3f} / {rev:.3f}")
    assert limited >= 0.02
    if N >= 31:
        assert fallback >= 0.02 and unlimited >= 0.02
        for share in (fwd, rev):
            assert 0.2 <= share <= 0.8  # adjacent and not adjacent: at least 20 % of the lanes each


@pytest.mark.parametrize("N,P,transport", C.DECOMPOSED, ids=[f"N{n}-P{p}" for n, p, _ in C.DECOMPOSED])
def test_one_plane_flow_keeps_the_row_branches(N, P, transport):
    """Scaling w changes k0, not the variety along a row: the decomposed cases still see both answers and all outcomes."""
    for dtype in C.DTYPES:
        u, v, w = C.mixed_flow_one_plane(N, dtype, N)
        fwd, rev = M.adjacency(u, v, w, DT)
        out = M.outcomes(C.normal_field(N, dtype, N), u, v, w, DT)
        print(f"N={N} {C.dname(dtype)}: outcomes {out} adjacent {fwd:.3f} / {rev:.3f}")
        assert min(out) >= 0.02 and 0.2 <= fwd <= 0.8 and 0.2 <= rev <= 0.8


# ---- a copy of the §9 reference in the form of the one-cell-per-lane kernel ---------------------------------------
def hw_min(p, q):
    """A hardware minimum (IEEE minNum, and -0 below +0) in place of SPEC §9's q < p ? q : p."""
    r = np.fmin(p, q)
    return np.where((p == 0) & (q == 0), np.where(np.signbit(p) | np.signbit(q), -abs(r), r), r)


def hw_max(p, q):
    r = np.fmax(p, q)
    return np.where((p == 0) & (q == 0), np.where(np.signbit(p) & np.signbit(q), r, abs(r)), r)


class McCopy:
    """SPEC §9 step 2 from gathered samples, the way advect_mc_row_kernel forms it: per cell the four i0 samples of d0
    (forward trace) and of hat (reverse trace), and the i0+1 samples either loaded by the cell itself or taken from the
    cell of the next lane where that cell's trace is adjacent. Unmutated it equals maccormack_ref.advect_mc in every bit
    (asserted by the test that uses it)."""

    def __init__(self, b, d0, u, v, w, dt, lanes=64):
        T = d0.dtype.type
        N = d0.shape[0] - 2
        self.b, self.d0, self.N, self.T = b, d0, N, T
        dt0 = T(dt) * T(N)
        self.hat = np.zeros_like(d0)
        O.advect(b, self.hat, d0, u, v, w, T(dt))
        self.F = M.trace_positions((u, v, w), dt0, -1)
        self.R = M.trace_positions((u, v, w), dt0, +1)
        lane = np.arange(N) % lanes
        self.has_next = np.broadcast_to((lane != lanes - 1) & (np.arange(N) < N - 1), (N, N, N))
        self.seam = np.broadcast_to((lane == lanes - 1) & (np.arange(N) < N - 1), (N, N, N))

    @staticmethod
    def pad(adj):
        return np.concatenate([adj, np.zeros(adj.shape[:2] + (1,), bool)], axis=2)

    def samples(self, field, idx, share):
        """(s0[4], s1[4]): corner c = (j0,k0), (j0,k1), (j1,k0), (j1,k1); s1 from the next cell's s0 where `share`."""
        i0, j0, k0 = idx
        s0 = [field[k0 + z, j0 + y, i0] for y, z in ((0, 0), (0, 1), (1, 0), (1, 1))]
        own = [field[k0 + z, j0 + y, i0 + 1] for y, z in ((0, 0), (0, 1), (1, 0), (1, 1))]
        nxt = [np.concatenate([a[:, :, 1:], a[:, :, -1:]], axis=2) for a in s0]
        return s0, [np.where(share, n, o) for n, o in zip(nxt, own)]

    def result(self, mutation=None):
        T, N, d0 = self.T, self.N, self.d0
        (fi, cf, _), (ri, cr, (xr, yr, zr)) = self.F, self.R
        share = []
        for idx in (fi, ri):
            adj = self.pad(M.next_cell_adjacent(idx)) & self.has_next
            if mutation == "i0_only":  # 1: j0 / k0 of the next cell not compared
                adj = self.pad(idx[0][:, :, 1:] == idx[0][:, :, :-1] + 1) & self.has_next
            if mutation == "lane63":  # 2: the last lane of a wave takes the next wave's first cell
                adj = adj | self.seam
            share.append(adj)
        hat = self.hat
        if mutation == "hat_shells":  # 5: bar from a hat whose shells were never set
            hat = np.zeros_like(hat)
            hat[I] = self.hat[I]
        a0, a1 = self.samples(d0, fi, share[0])
        h0, h1 = self.samples(hat, ri, share[1])
        mn_, mx_ = (hw_min, hw_max) if mutation == "hw_minmax" else (M.sel_min, M.sel_max)  # 3
        with np.errstate(invalid="ignore", over="ignore"):
            mn = mn_(mn_(mn_(a0[0], a0[1]), mn_(a0[2], a0[3])), mn_(mn_(a1[0], a1[1]), mn_(a1[2], a1[3])))
            mx = mx_(mx_(mx_(a0[0], a0[1]), mx_(a0[2], a0[3])), mx_(mx_(a1[0], a1[1]), mx_(a1[2], a1[3])))
            s1, t1, r1 = xr - ri[0].astype(T), yr - ri[1].astype(T), zr - ri[2].astype(T)
            s0, t0, r0 = T(1) - s1, T(1) - t1, T(1) - r1
            bar = (s0 * (t0 * (r0 * h0[0] + r1 * h0[1]) + t1 * (r0 * h0[2] + r1 * h0[3])) +
                   s1 * (t0 * (r0 * h1[0] + r1 * h1[1]) + t1 * (r0 * h1[2] + r1 * h1[3])))
            r = self.hat[I] + T(0.5) * (d0[I] - bar)
            r = np.where(r < mn, mn, r)
            r = np.where(r > mx, mx, r)
            r = np.where(cf if mutation == "cf_only" else (cf | cr), self.hat[I], r)  # 4
        assert r.dtype == d0.dtype
        d = np.zeros_like(d0)
        d[I] = r
        O.set_bnd(self.b, d)
        return d


MC_MUTATIONS = ("i0_only", "lane63", "hw_minmax", "cf_only", "hat_shells")
MC_SIZES = [N for N in C.SIZES if N <= 130]  # (the copy holds 16 gathered samples per cell: 200^3 adds nothing here)


def test_maccormack_mutations_are_caught():
    """Mutations 1-5. Cases: every size up to 130, both precisions, d0 standard normal ("plain") and d0 through
    special_values ("special"). The unmutated copy must equal the reference on every case."""
    caught = {m: [] for m in MC_MUTATIONS}
    for N in MC_SIZES:
        for dtype in C.DTYPES:
            u, v, w = C.mixed_flow(N, dtype, N)
            plain = C.normal_field(N, dtype, N)
            for kind, d0 in (("plain", plain), ("special", C.special_values(plain, np.random.RandomState(N)))):
                if kind == "special" and N not in (34, 70):
                    continue
                b = N % 4
                mc = McCopy(b, d0, u, v, w, DT)
                want = M.advect_mc(b, np.zeros_like(d0), d0, u, v, w, DT)
                case = f"N{N}-{C.dname(dtype)}-{kind}"
                assert same_bits(mc.result(), want), f"{case}: the copy is not the reference"
                for m in MC_MUTATIONS:
                    if not same_bits(mc.result(m), want):
                        caught[m].append(case)
    for m, cases in caught.items():
        print(f"{m}: caught by {' '.join(cases) or 'NOTHING'}")
    for m in MC_MUTATIONS:
        assert caught[m], f"no case catches mutation {m}"
    # a hardware min / max differs from the select form only on signed zeros and NaN: special_values, nothing else
    assert all(c.endswith("special") for c in caught["hw_minmax"])
    assert {c.split("-")[0] for c in caught["hw_minmax"]} == {"N34", "N70"}
    # the seam of two waves exists from 65 cells on
    assert {int(c.split("-")[0][1:]) for c in caught["lane63"]} == {65, 70, 130}
    # sizes 13 and up catch the rest in both precisions
    for m in ("i0_only", "cf_only", "hat_shells"):
        for N in (31, 34, 64, 65, 70, 130):
            assert {f"N{N}-f32-plain", f"N{N}-f64-plain"} <= set(caught[m]), (m, N)


def test_nan_and_inf_velocities_are_legal_inputs():
    """The velocities of the GPU special-value cases: NaN traces go to index 0 and infinities to a wall (SPEC §3); the
    reference is defined on them, and its result differs from that of the clean flow."""
    for N in (34, 70):
        for dtype in C.DTYPES:
            u, v, w = C.mixed_flow(N, dtype, N)
            rng = np.random.RandomState(N + 1)
            su, sv, sw = (C.special_values(c, rng) for c in (u, v, w))
            d0 = C.normal_field(N, dtype, N)
            a = M.advect_mc(0, np.zeros_like(d0), d0, su, sv, sw, DT)
            b = M.advect_mc(0, np.zeros_like(d0), d0, u, v, w, DT)
            assert not same_bits(a, b) and np.isfinite(a[I]).mean() > 0.9


# ---- §10 ---------------------------------------------------------------------------------------------------------
# (mutation 6, the row partial of one trip: ref_support.row_partials_one_trip)
def plane_partials_sequential(terms, W):
    """Mutation 7: the N row partials of a plane added one after another instead of folded by halving. (Padding to 2n
    instead of n cannot be told apart: the extra entries are +0.0 and no partial is ever -0.)"""
    R = D.row_partials(terms, W)
    p = np.zeros(R.shape[0], np.float64)
    for j in range(R.shape[1]):
        p = p + R[:, j]
    return p


def test_reduction_mutations_are_caught():
    caught = {"one_trip": [], "one_trip_dropped": [], "sequential_fold": []}
    for N, dtype in C.REDUCE_SHAPES:
        W = D.vec_width(dtype)
        x = C.decades_field(N, dtype, 300 + N)
        terms = x[I].astype(np.float64)
        want = D.plane_partials(terms, W)
        case = f"N{N}-{C.dname(dtype)}"
        for m, drop in (("one_trip", False), ("one_trip_dropped", True)):
            a = np.zeros((N, D.pad_pow2(N)), np.float64)
            a[:, :N] = row_partials_one_trip(terms, W, drop)
            if not np.array_equal(D.halve(a), want):
                caught[m].append(case)
        if not np.array_equal(plane_partials_sequential(terms, W), want):
            caught["sequential_fold"].append(case)
        twice = np.zeros((N, 2 * D.pad_pow2(N)), np.float64)
        twice[:, :N] = D.row_partials(terms, W)
        assert np.array_equal(D.halve(twice), want)  # padding further adds +0.0: no bit can change
    for m, cases in caught.items():
        print(f"{m}: caught by {' '.join(cases)}")
    # mutation 6: the m >= 1 sizes, all of them, and no smaller size. At N = 130 (fp64) and 260 (fp32) the second trip
    # holds one vector, lane 0's, which lane 0 adds after its first in either order: there only the dropped trip shows,
    # and the order of the second trip is checked by N = 200 (fp64) and 324 (fp32).
    assert caught["one_trip_dropped"] == [f"N{N}-{C.dname(t)}" for N, t in C.REDUCE_SHAPES if C.second_trip(N, t)]
    assert set(caught["one_trip_dropped"]) == {"N130-f64", "N200-f64", "N260-f32", "N324-f32"}
    assert caught["one_trip"] == ["N200-f64", "N324-f32"]
    # mutation 7: fp64 from 5 rows on; fp32 from 64 on (a short sum of fp32 terms spread over five decades is exact in
    # double, whatever its order)
    assert set(caught["sequential_fold"]) >= {f"N{N}-{C.dname(t)}" for N, t in C.REDUCE_SHAPES
                                              if N >= (5 if t == np.float64 else 64)}


# ---- §8 ----------------------------------------------------------------------------------------------------------
def add_forces_mutated(u, v, w, dens, su, sv, sw, eps, beta, ambient, axis, no_tiny=False, evaluate_zero=False):
    """forces_ref.confinement + add_forces with mutation 8: `tiny` left out of len + tiny, or a term whose coefficient
    is zero evaluated all the same."""
    N = u.shape[0] - 2
    s = F.scalars(N, u.dtype, eps, beta, ambient)
    cg, P_, M_, I_ = s["c_grad"], F.P, F.M, F.I
    src = (su, sv, sw)
    with np.errstate(all="ignore"):
        if s["eps"] != 0 or evaluate_zero:
            mag = F.vorticity(u, v, w)
            wx, wy, wz = F.curl(u, v, w, cg)
            ex = cg * (mag[I_, I_, P_] - mag[I_, I_, M_])
            ey = cg * (mag[I_, P_, I_] - mag[I_, M_, I_])
            ez = cg * (mag[P_, I_, I_] - mag[M_, I_, I_])
            ln = np.sqrt((ex * ex + ey * ey) + ez * ez)
            r = u.dtype.type(1) / (ln if no_tiny else ln + s["tiny"])
            nx, ny, nz = ex * r, ey * r, ez * r
            f = ((ny * wz) - (nz * wy), (nz * wx) - (nx * wz), (nx * wy) - (ny * wx))
            for a in range(3):
                src[a][I_, I_, I_] = src[a][I_, I_, I_] + s["eps_h"] * f[a]
        if s["beta"] != 0 or evaluate_zero:
            src[axis][I_, I_, I_] = src[axis][I_, I_, I_] + s["beta"] * (dens[I_, I_, I_] - s["amb"])


def test_force_mutations_are_caught():
    caught = {"no_tiny": [], "zero_term_evaluated": []}
    for N, dtype in C.SHAPES:
        case = f"N{N}-{C.dname(dtype)}"
        f = C.forces_fields(N, dtype, 11 + N)
        args = [f[n] for n in ("u", "v", "w", "dens")]
        want = [f[n].copy() for n in ("u0", "v0", "w0")]
        got = [f[n].copy() for n in ("u0", "v0", "w0")]
        copy = [f[n].copy() for n in ("u0", "v0", "w0")]
        F.add_forces(*args, *want, 0.35, 1.7, 0.1, 2)
        add_forces_mutated(*args, *copy, 0.35, 1.7, 0.1, 2)
        add_forces_mutated(*args, *got, 0.35, 1.7, 0.1, 2, no_tiny=True)
        assert all(same_bits(a, b) for a, b in zip(copy, want)), f"{case}: the copy is not the reference"
        assert all(np.isfinite(a).all() for a in want)
        if not all(same_bits(a, b) for a, b in zip(got, want)):
            caught["no_tiny"].append(case)
        z = C.zero_coefficient_inputs(N, dtype)
        args = [z[n] for n in ("u", "v", "w", "dens")]
        src = [z[n].copy() for n in ("u0", "v0", "w0")]
        F.add_forces(*args, *src, 0.0, 0.0, 0.1, 1)
        assert all(same_bits(a, z[n]) for a, n in zip(src, ("u0", "v0", "w0")))  # SPEC §8: nothing is evaluated
        add_forces_mutated(*args, *src, 0.0, 0.0, 0.1, 1, evaluate_zero=True)
        if not all(same_bits(a, z[n]) for a, n in zip(src, ("u0", "v0", "w0"))):
            caught["zero_term_evaluated"].append(case)
    for m, cases in caught.items():
        print(f"{m}: caught by {' '.join(cases)}")
    # len = 0 needs a region of uniform |omega|: the block of forces_fields (N >= 13), or N = 1 (SPEC §8.1)
    assert set(caught["no_tiny"]) == {f"N{N}-{C.dname(t)}" for N, t in C.SHAPES if N >= 13 or N == 1}
    assert len(caught["zero_term_evaluated"]) == len(C.SHAPES)
