"""The reference for Born modelling (csrc/born.hpp, sepfwi_born), shared by every test that compares it with the CPU oracle.

The reference package has nothing of the kind, so this is an unpinned extension.  The oracle's stencil kernels and helpers are
exported and take the media as arguments; they are linear in the fields, and linear in the media when the updated field starts at
zero.  So the scattered step needs no new C: this module is the oracle's forward shot loop (ofwi_shot, oracle/torchfwi_oracle.c)
restated as a Python step loop over the exported kernels (tests/oracle_loop.py) exactly as pseudo_hessian_ref._shot does it, and per
half-step
    (a) coupling term     the kernel on COPIES of the background's input fields and of its four C-PML memories of that half-step (taken
                          before the background half-step changes them), with the perturbed media (dlam, dmu, damu) resp. (dba, dbb) and
                          zeroed output fields: the output is the coupling term, with the background's C-PML-modified derivatives
    (b) propagation term  the kernel on the scattered fields (their own eight memories) with the background media
and (a) is added to the result of (b).  No source term.  The background loop's gathers equal oracle.cufd(..., calc_id 2) bit for bit
(tests/test_born_reference.py), which makes it the oracle's loop; the scattered gathers are confirmed there against central finite
differences of the oracle's gathers.

Perturbed media, float64 numpy from the oracle's own aMu, bA, bB (arrays [x][z]), cast to float32, zero outside [2, n-3]^2:
    dlam = 1e6 dLambda, dmu = 1e6 dMu
    damu = (aMu^2 / 4) sum_k dmu_k / mu_k^2  over (z,x), (z+1,x), (z,x+1), (z+1,x+1);  0 where aMu is 0
    dba  = -(bA^2 / 2) (dDen(z+1,x) + dDen(z,x)),   dbb = -(bB^2 / 2) (dDen(z,x+1) + dDen(z,x))
Either oracle build serves: both export the same kernels and helpers, and the loop run on the nvfma build (the reference binary's fused
multiply-adds inside the kernels) is a second valid rounding of the same arithmetic -- the yardstick of the fuzz tests.

born_side and shifted_gradient are what the tests of the Gauss-Newton product share: the gathers per shot and component, and the oracle's
gradient at the observed data obs_c = syn_c - (J v)_c -- a reference outside the GPU, where an error shared by sepfwi_born's two halves cannot cancel."""
import numpy as np

import gauge_ref as GA
import geophone_ref as GR
from fuzz_common import groups, l2
from oracle_loop import MEM_S, MEM_V, Setup, f32

COMPS = ("ett", "vx", "vz")
ROW = {"ett": 3, "vx": 1, "vz": 2}      # row of the component in the reference's gathers [pr, vx, vz, ett]
GRADS = ("gLambda", "gMu", "gDen")


def delta_media(media, dLambda, dMu, dDen):
    """The five perturbed-media arrays [x][z] float32 (module docstring) from oracle_loop.internal_media's tuple and dense (nz, nx) v."""
    fLam, fMu, fDen, aMu, bA, bB = media
    nx, nz = fMu.shape
    dlam = (f32(dLambda).T.astype(np.float64) * 1e6)
    dmu = (f32(dMu).T.astype(np.float64) * 1e6)
    dden = f32(dDen).T.astype(np.float64)
    damu, dba, dbb = [np.zeros((nx, nz), np.float64) for _ in range(3)]
    xs, zs = slice(2, nx - 2), slice(2, nz - 2)
    sh = lambda a, kx, kz: a[xs.start + kx:xs.stop + kx, zs.start + kz:zs.stop + kz]
    mu64 = fMu.astype(np.float64)
    am = aMu[xs, zs].astype(np.float64)
    s = np.zeros_like(am)
    with np.errstate(divide="ignore", invalid="ignore"):
        for kx, kz in ((0, 0), (0, 1), (1, 0), (1, 1)):
            s += np.where(am != 0.0, sh(dmu, kx, kz) / sh(mu64, kx, kz) ** 2, 0.0)
    damu[xs, zs] = np.where(am != 0.0, am * am / 4.0 * s, 0.0)
    dba[xs, zs] = -(bA[xs, zs].astype(np.float64) ** 2) / 2.0 * (sh(dden, 0, 1) + sh(dden, 0, 0))
    dbb[xs, zs] = -(bB[xs, zs].astype(np.float64) ** 2) / 2.0 * (sh(dden, 1, 0) + sh(dden, 0, 0))
    return f32(dlam), f32(dmu), f32(damu), f32(dba), f32(dbb)


def _shot(s, dmedia, stf, z_src, x_src, z_rec, x_rec, sens, terms=(True, True, True)):
    """Forward loop of one shot of the call s (oracle_loop.Setup), background and scattered field.  -> syn, dsyn (4, nrec, nSteps) each.
    terms: switches for the (lam/mu, amu, density) coupling terms -- all on, except in tests that show what a dropped term costs."""
    dlam, dmu, damu, dba, dbb = dmedia
    zero = np.zeros((s.nx, s.nz), np.float32)
    if not terms[0]:
        dlam, dmu = zero, zero
    if not terms[1]:
        damu = zero
    if not terms[2]:
        dba, dbb = zero, zero
    f, d, t = s.new_fields(), s.new_fields(), s.new_fields()      # background, scattered, the coupling term's scratch set
    syn = np.zeros((4, z_rec.size, s.nSteps), np.float32)
    dsyn = np.zeros_like(syn)
    for it in range(s.nSteps - 1):
        # ---- stress half-step: (a) on copies of the background's velocities and stress-side memories, (b), then the background
        for k in ("vz", "vx") + MEM_S:
            t[k][:] = f[k]
        for k in ("szz", "sxx", "sxz"):
            t[k][:] = 0.0
        s.stress(t, dlam, dmu, damu)
        s.stress(d, s.fLam, s.fMu, s.aMu)
        for k in ("szz", "sxx", "sxz"):
            d[k] += t[k]
        s.stress(f, s.fLam, s.fMu, s.aMu)
        s.add_source(f, stf[it], z_src, x_src)                        # (the background only)
        # ---- velocity half-step: the background's stresses after update and source add
        for k in ("szz", "sxx", "sxz") + MEM_V:
            t[k][:] = f[k]
        for k in ("vz", "vx"):
            t[k][:] = 0.0
        s.velocity(t, dba, dbb)
        s.velocity(d, s.bA, s.bB)
        for k in ("vz", "vx"):
            d[k] += t[k]
        s.velocity(f, s.bA, s.bB)
        s.record(syn, it + 1, f, z_rec, x_rec, sens)
        s.record(dsyn, it + 1, d, z_rec, x_rec, sens)
    return syn, dsyn


def born(oracle, Lambda, Mu, Den, dLambda, dMu, dDen, Stf, shot_ids, para, survey, terms=(True, True, True), stack=True):
    """oracle.cufd's model arguments plus the perturbation (dense (nz, nx) each).  One-cell horizontal or vertical channels and
    directional ones (no gauge length: tests expand gauges into their member channels).
    -> dict(syn, dsyn: (nshots, 4, nrec, nSteps) background and scattered gathers [pr, vx, vz, ett]; dmedia: the five arrays [x][z]).
    stack=False: syn and dsyn are lists with one (4, nrec, nSteps) array per shot -- the shots may then have different channel counts."""
    s = Setup(oracle, Lambda, Mu, Den, para)
    dmed = delta_media(s.media, dLambda, dMu, dDen)
    syn_all, dsyn_all = [], []
    for sid, stf_s, z_src, x_src, z_rec, x_rec, _, sens in s.shots(Stf, shot_ids, survey):
        syn, dsyn = _shot(s, dmed, stf_s, z_src, x_src, z_rec, x_rec, sens, terms)
        syn_all.append(syn)
        dsyn_all.append(dsyn)
    if not stack:
        return dict(syn=syn_all, dsyn=dsyn_all, dmedia=dmed)
    return dict(syn=np.stack(syn_all), dsyn=np.stack(dsyn_all), dmedia=dmed)


def perturbation(pb, seed=3, scale=0.01, only=None, model="lame_init", water_rows=0):
    """A smooth random v = (dLambda, dMu, dDen) over the whole padded grid (PML included), about `scale` of the model's size, every
    parameter non-zero; only = 0 / 1 / 2: that parameter alone.  float32 numpy (nz, nx).  With `water_rows` rows of water on top dMu is
    zero in them: a fluid stays a fluid (the harmonic mean of mu is not differentiable at mu = 0)."""
    import problems as P
    rng = np.random.default_rng(seed)
    out = []
    for k, m in enumerate(pb[model]):
        m = m.numpy()
        a = P.smooth_random(rng, m.shape, -1.0, 1.0, passes=6) * scale * float(np.abs(m).mean())
        out.append(f32(a if only is None or only == k else np.zeros_like(a)))
    out[1][:int(water_rows)] = 0.0
    return out


def water_problem(tmp, name):
    """Problem A of the pseudo-Hessian tests, or W: the same with water over the top 12 physical rows (source in the water, fibre below
    the sea bed, as tests/test_gpu_parity.py::test_water_layer_mu_zero builds it).  -> (problem, first row below the water)."""
    import problems as P
    from pseudo_hessian_ref import PROBLEM_A
    kw = dict(PROBLEM_A)
    if name == "W":
        kw.update(src_z=5, rec_z=22)
    pb = P.make_problem(str(tmp), **kw)
    w = 0
    if name == "W":
        w = pb["nPml"] + 12
        P.add_water(pb, w)
    return pb, w


# ---- the Gauss-Newton product's reference: the oracle's gradient at shifted data ---------------------------------------------------
def born_side(lib, pb, sv, b, m, v):
    """born_ref on one oracle build -> per shot {component: (nrec, nSteps)} of the background (syn) and the scattered (dsyn) gathers;
    with a gauge length the strain is the weighted mean of the member channels' (float64) and vx / vz are the centre member's."""
    stf, ids = pb["Stf"].numpy(), pb["Shot_ids"].numpy()
    G = b["G"]
    if G:
        plain = {k: val for k, val in pb["para"].items() if k != "das_gauge_length"}
        r = born(lib, *m, *v, stf, ids, plain, GA.member_survey(sv, G, b["vertical"]), stack=False)
        pick = lambda a: dict(ett=GA.gauge_of(a[3][None], G)[0], vx=GA.centre_of(a[1][None], G)[0], vz=GA.centre_of(a[2][None], G)[0])
    else:
        r = born(lib, *m, *v, stf, ids, pb["para"], sv, stack=False)
        pick = lambda a: {c: a[ROW[c]] for c in COMPS}
    return [pick(a) for a in r["syn"]], [pick(a) for a in r["dsyn"]], r


def shifted_gradient(lib, pb, sv, b, m, syn, dsyn):
    """The oracle's gradient at obs_c = syn_c - (J v)_c (float32 data, as a file would hold them) on one build.
    -> dict(gLambda, gMu, gDen (float64 sums over the shot groups), misfit, E: 0.5 sum w_c |obs_c|^2, jv2: |W^1/2 J v|^2)."""
    stf, ids = pb["Stf"].numpy(), [int(i) for i in pb["Shot_ids"].tolist()]
    para, G, weights = pb["para"], b["G"], b["weights"]
    w = dict(zip(COMPS, weights or (1.0, 0.0, 0.0)))
    obs = [{c: (np.asarray(s[c], np.float64) - np.asarray(ds[c], np.float64)).astype(np.float32) for c in COMPS} for s, ds in zip(syn, dsyn)]
    E = 0.5 * sum(w[c] * l2(o[c]) ** 2 for o in obs for c in COMPS if w[c] > 0)
    jv2 = sum(w[c] * l2(ds[c][:, 1:]) ** 2 for ds in dsyn for c in COMPS if w[c] > 0)
    out = {k: 0.0 for k in GRADS}
    misfit = 0.0
    if G:
        r = GA.reference(lib, m, stf, np.asarray(ids, np.int32), para, sv, G, [o["ett"] for o in obs])
        out = {k: r[k].astype(np.float64) for k in GRADS}
        misfit = r["misfit"]
    else:
        for grp in groups(ids, sv):
            pos = [ids.index(i) for i in grp]
            full = np.zeros((len(grp), 4) + obs[pos[0]]["ett"].shape, np.float32)
            for j, p in enumerate(pos):
                for c in COMPS:
                    full[j, ROW[c]] = obs[p][c]
            if weights:
                r = GR.cufd(lib, *m, stf, 1, grp, para, sv, obs=full, weights=weights)
            else:
                r = lib.cufd(*m, stf, 1, np.asarray(grp, np.int32), para, sv, obs=full)
            for k in GRADS:
                out[k] = out[k] + r[k].astype(np.float64)
            misfit += float(r["misfit"])
    out.update(misfit=misfit, E=E, jv2=jv2)
    return out
