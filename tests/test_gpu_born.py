"""Born modelling J v and the Gauss-Newton product J^T W J v on the GPU (-m gpu): csrc/born.hip and csrc/session_born.cpp through
sepfwi_born and fwi_ops.born / gauss_newton, against the scattered field of the CPU oracle's own kernels (tests/born_ref.py, which
tests/test_born_reference.py confirms against finite differences of the oracle's gathers).

Tolerance against the reference, per component: the suite's seismogram tolerance (README parity statement) -- max-norm deviation
<= 1e-4 of the component's maximum and rel-L2 <= 1e-4.  A dropped coupling term is an error of 0.35 ... 1.0, a wrong averaging
derivative several 1e-2 (tests/test_born_reference.py).

Measured on the MI355X (profiles/r09_born.txt): see the prints of each test."""
import ctypes as C

import numpy as np
import pytest
import torch

import born_ref as B
import fuzz_common as FC
import problems as P
import pseudo_hessian_ref as R
from born_ref import COMPS, GRADS, ROW, born_side, shifted_gradient
from fuzz_common import write_para
from gauge_ref import gauge_of, member_survey
from sepfwi import utils as ft

pytestmark = pytest.mark.gpu
TOL = 1e-4
PROBLEM_B3 = dict(R.PROBLEM_B, nshots=3)    # 40 x 150, three row segments, three Born shots in a row in one session
LINEARITY_REF = 4.8e-7                      # born_ref(2 v) against 2 born_ref(v), tests/test_born_reference.py


def gpu_born(hip_ops, pb, v, para_fname=None, ids=None, components=COMPS):
    """-> {component: (nshots, nrec, nSteps) float32 numpy}"""
    out = hip_ops.born(*[t.cuda() for t in pb["lame_init"]], *[torch.from_numpy(a).cuda() for a in v], pb["Stf"], 1,
                       pb["Shot_ids"] if ids is None else ids, para_fname or pb["para_fname"], components=components)
    return {c: np.stack([d[c].cpu().numpy() for d in out]) for c in components}


def ref_born(oracle, pb, v, para=None, survey=None):
    return B.born(oracle, *[t.numpy() for t in pb["lame_init"]], *v, pb["Stf"].numpy(), pb["Shot_ids"].numpy(), para or pb["para"],
                  survey or pb["survey"])["dsyn"]


def close(got, ref, what):
    """got {component: (nshots, nrec, nSteps)} against the reference's (nshots, 4, nrec, nSteps)"""
    worst = {}
    for c in got:
        w = np.asarray(ref[:, ROW[c]], np.float64)
        g = got[c]
        assert g.shape == w.shape and np.isfinite(g).all() and np.abs(w).max() > 0, (what, c)
        worst[c] = (np.abs(g - w).max() / np.abs(w).max(), P.rel_l2(g, w))
        print("born %s, d%s: max-norm deviation %.2e of the maximum, rel-L2 %.2e" % (what, c, worst[c][0], worst[c][1]))
    for c, (dmax, l2) in worst.items():
        assert dmax <= TOL and l2 <= TOL, (what, c, dmax, l2)


@pytest.fixture(scope="module")
def prob_a(oracle, hip_ops, tmp_path_factory):
    """50 x 90 (two row segments, the last ragged), two shots; v: all three parameters; the reference of the joint v."""
    pb = P.make_problem(str(tmp_path_factory.mktemp("born_a")), **R.PROBLEM_A)
    v = B.perturbation(pb)
    return pb, v, ref_born(oracle, pb, v)


def test_scattered_gathers_match_the_reference_50x90(hip_ops, prob_a):
    """1: ett, vx, vz of J v, two shots, C-PML on all four sides."""
    pb, v, ref = prob_a
    close(gpu_born(hip_ops, pb, v), ref, "50x90")


def test_scattered_gathers_match_the_reference_40x150_three_shots(oracle, hip_ops, tmp_path):
    """1: three row segments, three shots one after the other in one session (the scattered fields and their C-PML memories restart
    from zero for every shot), and the second call of the session gives the same bits as the first."""
    pb = P.make_problem(str(tmp_path), **PROBLEM_B3)
    v = B.perturbation(pb, seed=5)
    got = gpu_born(hip_ops, pb, v)
    close(got, ref_born(oracle, pb, v), "40x150")
    again = gpu_born(hip_ops, pb, v)
    for c in COMPS:
        assert np.array_equal(got[c], again[c]), c
    last = gpu_born(hip_ops, pb, v, ids=torch.tensor([2], dtype=torch.int32))     # shot 2 alone = shot 2 after shots 0 and 1
    for c in COMPS:
        assert np.array_equal(got[c][2:], last[c]), c


def test_each_parameter_alone_and_their_sum(oracle, hip_ops, prob_a):
    """2: v = (dLambda, 0, 0), (0, dMu, 0), (0, 0, dDen) each against the reference; their sum against the joint run to round-off.
    The bound is the reference's own: the deviation of the sum of born_ref's three runs from its joint run (float32 round-off of
    three field sets against one, measured here on the CPU), or born_ref's linearity deviation if that is larger, times 4."""
    pb, v, ref = prob_a
    joint = gpu_born(hip_ops, pb, v)
    got_sum = {c: np.zeros_like(joint[c], dtype=np.float64) for c in COMPS}
    ref_sum = np.zeros(ref.shape, np.float64)
    for k, name in enumerate(("dLambda", "dMu", "dDen")):
        vk = [a if j == k else np.zeros_like(a) for j, a in enumerate(v)]
        rk = ref_born(oracle, pb, vk)
        gk = gpu_born(hip_ops, pb, vk)
        close(gk, rk, "50x90 " + name + " alone")
        ref_sum += rk
        for c in COMPS:
            got_sum[c] += gk[c]
    for c in COMPS:
        ref_dev = np.abs(ref_sum[:, ROW[c]] - ref[:, ROW[c]]).max() / np.abs(ref[:, ROW[c]]).max()
        dev = np.abs(got_sum[c] - joint[c]).max() / np.abs(joint[c]).max()
        bound = 4.0 * max(ref_dev, LINEARITY_REF)
        print("born sum of the three single-parameter runs against the joint run, d%s: %.2e of the maximum (reference %.2e, bound %.2e)" % (c, dev, ref_dev, bound))
        assert dev <= bound, (c, dev, bound)


@pytest.mark.parametrize("kind", ["strided", "vertical", "directional"])
def test_receiver_geometries_match_the_reference(tmp_path, oracle, hip_ops, kind):
    """3: scattered channels (every third cell: not a line, k_record), a vertical fibre, directional channels -- the scattered gathers
    are the matching linear samples of the reference's scattered fields."""
    kw = dict(R.PROBLEM_A, **{"strided": dict(nrec_stride=3), "vertical": dict(das_fiber="vertical"), "directional": dict(das_sensitivity="random", nrec_stride=2)}[kind])
    pb = P.make_problem(str(tmp_path), **kw)
    v = B.perturbation(pb, seed=11)
    close(gpu_born(hip_ops, pb, v), ref_born(oracle, pb, v), "50x90 " + kind)


def test_gauge_length_is_the_mean_of_the_member_channels(tmp_path, oracle, hip_ops):
    """3: das_gauge_length with G = 3.  The gauge's scattered strain equals the weighted mean of its member channels' -- of the
    reference's scattered field sampled on the member survey (gauge_ref.member_survey), and vx / vz are those of the channel's own cell."""
    G = 3
    pb = P.make_problem(str(tmp_path), **dict(R.PROBLEM_A, nrec_stride=2))
    fn, _ = write_para(pb, "gauge", das_gauge_length=G * pb["para"]["dx"])
    v = B.perturbation(pb, seed=13)
    got = gpu_born(hip_ops, pb, v, para_fname=fn)
    members = ref_born(oracle, pb, v, survey=member_survey(pb["survey"], G, False))      # (nshots, 4, nrec * G, nSteps)
    ref = np.zeros((members.shape[0], 4, members.shape[2] // G, members.shape[3]), np.float64)
    ref[:, 3] = gauge_of(members[:, 3], G)
    for k in (1, 2):
        ref[:, k] = members[:, k].reshape(members.shape[0], -1, G, members.shape[3])[:, :, G // 2]
    close(got, ref, "50x90 gauge 3")


def test_a_born_call_leaves_the_session_as_it_found_it(hip_ops, prob_a):
    """4: a gradient call before and after a Born call (and a Gauss-Newton product) returns the same bits; the session allocates
    nothing for Born modelling before the first Born call; the background field of the Born pass is the plain forward pass's, bit
    for bit (all five fields at the last step, sepfwi_debug_field)."""
    pb, v, _ = prob_a
    hip_ops.release()
    m = [t.cuda() for t in pb["lame_init"]]
    tv = [torch.from_numpy(a).cuda() for a in v]
    hip_ops.obscalc(*[t.cuda() for t in pb["lame_true"]], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], to_store=True)
    before = hip_ops.backward(*m, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    bytes0 = hip_ops.stats(pb["para_fname"])["device_bytes"]
    again = hip_ops.backward(*m, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    assert hip_ops.stats(pb["para_fname"])["device_bytes"] == bytes0
    parts = hip_ops.misfit_parts(pb["para_fname"])
    hip_ops.born(*m, *tv, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], components=COMPS)
    assert hip_ops.stats(pb["para_fname"])["device_bytes"] > bytes0
    hip_ops.gauss_newton(*m, *tv, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    assert hip_ops.misfit_parts(pb["para_fname"]) == parts
    after = hip_ops.backward(*m, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    for a, b, c in zip(before, again, after):
        assert torch.equal(a.cpu(), b.cpu()) and torch.equal(a.cpu(), c.cpu())
    one = torch.tensor([1], dtype=torch.int32)
    with P.kernel_options(batch=0):
        hip_ops.forward(*m, pb["Stf"], 0, one, pb["para_fname"])
        plain = [hip_ops.debug_field(pb["para_fname"], k) for k in range(5)]
    hip_ops.born(*m, *tv, pb["Stf"], 1, one, pb["para_fname"])
    for k in range(5):
        f = hip_ops.debug_field(pb["para_fname"], k)
        assert plain[k].abs().max() > 0 and torch.equal(f, plain[k]), k
    assert hip_ops.debug_field(pb["para_fname"], 10).abs().max() > 0      # the scattered vz


def gn_against_backward(hip_ops, pb, v, weights, tag):
    """hv = gauss_newton(m, v) in one session against backward at m in a second session whose observed data are syn(m) - J v, both
    from the GPU.  -> (measured deviations per array relative to its maximum, the bound)."""
    keys = {} if weights == (1.0, 0.0, 0.0) else dict(misfit_w_ett=weights[0], misfit_w_vx=weights[1], misfit_w_vz=weights[2])
    fn_gn, _ = write_para(pb, "gn_" + tag, **keys)
    fn_bw, para_bw = write_para(pb, "bw_" + tag, **keys)
    m = [t.cuda() for t in pb["lame_init"]]
    tv = [torch.from_numpy(a).cuda() for a in v]
    ids, nS = pb["Shot_ids"], pb["nSteps"]
    hv = [t.cpu().numpy() for t in hip_ops.gauss_newton(*m, *tv, pb["Stf"], 1, ids, fn_gn)]
    jv = gpu_born(hip_ops, pb, v, para_fname=fn_gn)
    hip_ops.obscalc(*m, pb["Stf"], 1, ids, fn_bw)                           # syn(m) as Shot_*.bin of the second session's directory
    active = [c for c, w in zip(COMPS, weights) if w > 0]
    noise, norm2 = 0.0, 0.0
    for i, sid in enumerate(ids.tolist()):
        for c, w in zip(COMPS, weights):
            if w <= 0:
                continue
            syn = ft.read_shot_gather(para_bw["data_dir_name"], c, sid, nS)
            hip_ops.set_observed_component(fn_bw, sid, c, torch.from_numpy((syn - jv[c][i]).astype(np.float32)))
            # float32: obs = fl(syn - Jv) carries half an ulp of |syn|, obs - syn another; relative to the adjoint source's size
            noise = max(noise, 1e-7 * float(np.abs(syn).max()) / float(np.abs(jv[c][i]).max()))
            norm2 += w * float((jv[c][i].astype(np.float64) ** 2).sum())
    out = hip_ops.backward(*m, pb["Stf"], 1, ids, fn_bw)
    g = [t.cpu().numpy() for t in out[1:4]]
    vhv = sum(float((a.astype(np.float64) * b.astype(np.float64)).sum()) for a, b in zip(v, hv))
    print("gauss-newton %s weights %s (components %s): v^T H v = %.6e, |W^1/2 J v|^2 = %.6e, ratio %.4f" % (tag, weights, active, vhv, norm2, vhv / norm2))
    dev = []
    for name, a, b in zip(("hvLambda", "hvMu", "hvDen"), hv, g):
        assert np.isfinite(a).all() and np.abs(b).max() > 0
        dev.append(float(np.abs(a - b).max() / np.abs(b).max()))
        print("gauss-newton %s %s: deviation from the gradient at obs = syn - J v %.2e of its maximum (bound %.2e = 10 x %.2e)" % (tag, name, dev[-1], 10 * noise, noise))
    stats = hip_ops.stats(fn_gn)
    return dev, 10.0 * noise, stats


@pytest.mark.parametrize("weights", [(1.0, 0.0, 0.0), (1.0, 0.5, 0.25)])
def test_gauss_newton_product_is_the_gradient_at_shifted_data_small_grid(hip_ops, prob_a, weights):
    """5: 50 x 90, too small for the persistent loop -- the product's backward half runs the two-launch step."""
    pb, v, _ = prob_a
    hip_ops.release()
    dev, bound, _ = gn_against_backward(hip_ops, pb, v, weights, "small%d" % (weights != (1.0, 0.0, 0.0)))
    assert max(dev) <= bound, (dev, bound)


@pytest.mark.parametrize("weights", [(1.0, 0.0, 0.0), (1.0, 0.5, 0.25)])
def test_gauss_newton_product_through_the_persistent_loop(tmp_path, hip_ops, weights):
    """5: 300 x 500 with bwd_fuse = 4: the backward half of the product is the persistent loop (persist_steps == nSteps - 1)."""
    hip_ops.release()
    pb = P.make_problem(str(tmp_path), nz=300, nx=500, nPml=10, nSteps=420, nshots=1, hetero=True, rec_z=40)
    v = B.perturbation(pb, seed=17)
    with P.kernel_options(bwd_fuse=4):
        keys = {} if weights == (1.0, 0.0, 0.0) else dict(misfit_w_ett=weights[0], misfit_w_vx=weights[1], misfit_w_vz=weights[2])
        fn, _ = write_para(pb, "loop", **keys)
        hip_ops.gauss_newton(*[t.cuda() for t in pb["lame_init"]], *[torch.from_numpy(a).cuda() for a in v], pb["Stf"], 1, pb["Shot_ids"], fn)
        st = hip_ops.stats(fn)
        assert st["persist_steps"] == pb["nSteps"] - 1, (st["persist_steps"], hip_ops.loop_status(fn))
        dev, bound, _ = gn_against_backward(hip_ops, pb, v, weights, "loop%d" % (weights != (1.0, 0.0, 0.0)))
    assert max(dev) <= bound, (dev, bound)
    hip_ops.release()


def test_refusals_are_error_codes(tmp_path, hip_ops):
    """6: NULL dLambda, a shape mismatch from Python, ngpu = 2, the product with a live conditioning key -- each an error, none a fault;
    under the conditioning key the scattered gathers alone are still served, and they are the unconditioned ones."""
    from sepfwi import _native
    pb = P.make_problem(str(tmp_path), nz=40, nx=48, nPml=10, nSteps=120, nshots=1)
    v = B.perturbation(pb)
    m = [t.cuda() for t in pb["lame_init"]]
    tv = [torch.from_numpy(a).cuda() for a in v]
    L = _native.lib()
    ids = np.zeros(1, np.int32)
    out = torch.zeros(pb["nrec"] * pb["nSteps"], dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    stf = pb["Stf"].contiguous()
    rc = L.sepfwi_born(p(out), None, None, None, None, None, p(m[0]), p(m[1]), p(m[2]), None, p(tv[1]), p(tv[2]), p(stf), 0, 1,
                       C.c_void_p(ids.ctypes.data), pb["para_fname"].encode(), None)
    assert rc == -1 and b"dLambda" in L.sepfwi_last_error()
    rc = L.sepfwi_born(p(out), None, None, p(m[0].clone()), None, None, p(m[0]), p(m[1]), p(m[2]), p(tv[0]), p(tv[1]), p(tv[2]), p(stf), 0, 1,
                       C.c_void_p(ids.ctypes.data), pb["para_fname"].encode(), None)
    assert rc == -1 and b"hv_" in L.sepfwi_last_error()
    with pytest.raises(ValueError, match="one shape"):
        hip_ops.born(*m, tv[0][:-1], tv[1], tv[2], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    with pytest.raises(TypeError, match="float32"):
        hip_ops.born(*m, tv[0].double(), tv[1], tv[2], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    with pytest.raises(ValueError, match="ONE GPU"):
        hip_ops.born(*m, *tv, pb["Stf"], 2, pb["Shot_ids"], pb["para_fname"])
    with pytest.raises(ValueError, match="ONE GPU"):
        hip_ops.gauss_newton(*m, *tv, pb["Stf"], 2, pb["Shot_ids"], pb["para_fname"])
    fn, _ = write_para(pb, "cond", if_cross_misfit=True)
    with pytest.raises(_native.SepFwiError) as e:
        hip_ops.gauss_newton(*m, *tv, pb["Stf"], 1, pb["Shot_ids"], fn)
    assert e.value.code == -1 and "conditioned" in str(e.value)
    plain = gpu_born(hip_ops, pb, v)
    cond = gpu_born(hip_ops, pb, v, para_fname=fn)
    for c in COMPS:
        assert np.abs(plain[c]).max() > 0 and np.array_equal(plain[c], cond[c]), c
    hv = hip_ops.gauss_newton(*m, *tv, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])      # the session still works
    assert all(torch.isfinite(h).all() and h.abs().max() > 0 for h in hv)


# ---- water, kernel structures, the pseudo-Hessian, img_every --------------------------------------------------------------------
def product_against_the_oracle(oracle, oracle_nvfma, pb, v, hv, water, tag):
    """hv (three numpy arrays) against the oracle's gradient at obs = syn - J v formed from born_ref on the CPU, on both oracle builds:
    the bound and the yardstick of tests/test_gpu_born_fuzz.py (tests/fuzz_common.py)."""
    b = dict(G=0, vertical=False, weights=None)
    m = [t.numpy() for t in pb["lame_init"]]
    sides = []
    for lib in (oracle, oracle_nvfma):
        syn, dsyn, _ = born_side(lib, pb, pb["survey"], b, m, v)
        sides.append(shifted_gradient(lib, pb, pb["survey"], b, m, syn, dsyn))
    ref, alt = sides
    cond_g = FC.conditioning(ref["E"], ref["misfit"])[1]
    for name, g in zip(GRADS, hv):
        r, a = ref[name], alt[name]
        print("gauss-newton %s hv%s: rel-L2 deviation from the oracle's gradient at obs = syn - J v %.2e (the two oracle builds %.2e, cond_g %.1e)"
              % (tag, name[1:], FC.rel(FC.d_own(g, r), r), FC.rel(FC.d_own(a, r), r), cond_g))
    for name, g in zip(GRADS, hv):
        assert np.isfinite(g).all() and FC.l2(ref[name]) > 0, (tag, name)
        miss = FC.gradient_miss(g, ref[name], alt[name], FC.GRAD_TOL, cond_g, water, FC.d_own)
        assert not miss, (tag, name, miss)


def test_water_layer_50x90(tmp_path, oracle, oracle_nvfma, hip_ops):
    """Problem W of tests/test_born_reference.py: 22 rows of water (mu = 0) on top, the source in the water, the fibre below the sea
    bed; dMu = 0 in the water.  The gathers against the reference; the scattered sxz is exactly 0 wherever one of the four mu taps of
    its average is a fluid cell (the am != 0 guard of k_born_media next to the average rebuilt on the fly); the product against the
    oracle's gradient at shifted data."""
    pb, w = B.water_problem(tmp_path, "W")
    v = B.perturbation(pb, water_rows=w)
    hip_ops.release()
    close(gpu_born(hip_ops, pb, v), ref_born(oracle, pb, v), "50x90 water")
    sxz = hip_ops.debug_field(pb["para_fname"], 14).numpy()
    mu = np.pad(pb["lame_init"][1].numpy(), ((0, 1), (0, 1)), mode="edge")
    nzc, nx = sxz.shape
    fluid = (mu[:nzc, :nx] == 0) | (mu[1:nzc + 1, :nx] == 0) | (mu[:nzc, 1:nx + 1] == 0) | (mu[1:nzc + 1, 1:nx + 1] == 0)
    assert fluid[:w].all() and not fluid[w:].any()
    assert np.isfinite(sxz).all() and np.abs(sxz[~fluid]).max() > 0
    assert not np.any(sxz[fluid]), "scattered sxz in the water: %.3e" % np.abs(sxz[fluid]).max()
    hv = hip_ops.gauss_newton(*[t.cuda() for t in pb["lame_init"]], *[torch.from_numpy(a).cuda() for a in v], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    product_against_the_oracle(oracle, oracle_nvfma, pb, v, [h.cpu().numpy() for h in hv], w, "50x90 water")


def _born_bits(hip_ops, pb, v, fn):
    """gathers, the five background fields after the last shot's last step, hv -- of one session under the options in force"""
    m = [t.cuda() for t in pb["lame_init"]]
    tv = [torch.from_numpy(a).cuda() for a in v]
    got = gpu_born(hip_ops, pb, v, para_fname=fn)
    fields = [hip_ops.debug_field(fn, k) for k in range(5)]
    hv = [t.cpu() for t in hip_ops.gauss_newton(*m, *tv, pb["Stf"], 1, pb["Shot_ids"], fn)]
    return got, fields, hv


def test_kernel_structures_give_the_default_structure_s_bits(probes_lib, hip_ops, prob_a):
    """bz in {1, 4, 8}, xcd_remap = 0 and rk_lazy = 0 change which thread updates which cell and when a C-PML coefficient is loaded,
    not one operation on a value: Born gathers, background fields and the product equal the default structure's bit for bit (all on
    the probes build of the library, which alone exposes these options).
    rho_fly = 0 and amu_fly = 0 read the stored averages instead of rebuilding them (for mu another rounding): there the background
    equals a plain forward pass under the same option bit for bit, and the gathers meet the tolerance against the reference."""
    pb, v, ref = prob_a
    fn, _ = write_para(pb, "structures")
    m = [t.cuda() for t in pb["lame_init"]]
    tv = [torch.from_numpy(a).cuda() for a in v]
    with P.kernel_options():
        assert all(probes_lib.sepfwi_get_option(k.encode()) == P.OPTION_DEFAULTS[k] for k in ("bz", "xcd_remap", "rk_lazy", "rho_fly", "amu_fly"))
        base = _born_bits(hip_ops, pb, v, fn)
    assert all(f.abs().max() > 0 for f in base[1]) and all(h.abs().max() > 0 for h in base[2])
    for opts in (dict(bz=1), dict(bz=4), dict(bz=8), dict(xcd_remap=0), dict(rk_lazy=0)):
        with P.kernel_options(**opts):
            assert all(probes_lib.sepfwi_get_option(k.encode()) == val for k, val in opts.items()), (opts, "the option is not in force")
            got, fields, hv = _born_bits(hip_ops, pb, v, fn)
        for c in COMPS:
            assert np.array_equal(got[c], base[0][c]), (opts, c)
        for k in range(5):
            assert torch.equal(fields[k], base[1][k]), (opts, "background field %d" % k)
        for k in range(3):
            assert torch.equal(hv[k], base[2][k]), (opts, "hv %d" % k)
    hip_ops.obscalc(*[t.cuda() for t in pb["lame_true"]], pb["Stf"], 1, pb["Shot_ids"], fn, to_store=True)
    last = pb["Shot_ids"][-1:].clone()
    for opts in (dict(rho_fly=0), dict(amu_fly=0)):
        with P.kernel_options(batch=0, **opts):
            assert all(probes_lib.sepfwi_get_option(k.encode()) == val for k, val in opts.items()), (opts, "the option is not in force")
            hip_ops.forward(*m, pb["Stf"], 0, last, fn)
            plain = [hip_ops.debug_field(fn, k) for k in range(5)]
            got = gpu_born(hip_ops, pb, v, para_fname=fn)
            for k in range(5):
                assert plain[k].abs().max() > 0 and torch.equal(hip_ops.debug_field(fn, k), plain[k]), (opts, "background field %d" % k)
        close(got, ref, "50x90 %r" % (opts,))
        if "amu_fly" in opts:   # (the stored average is the double-precision one, the rebuilt one uses the hardware reciprocal; the stored
            # buoyancies are the rebuilt ones' bits, so rho_fly = 0 changes where a value comes from and not the value)
            assert any(not np.array_equal(got[c], base[0][c]) for c in COMPS), (opts, "the option changed nothing: it was not in force")


def test_born_calls_leave_the_pseudo_hessian_untouched(hip_ops, prob_a):
    """The pseudo-Hessian of an armed gradient call, read again after a Born call and a product: the bits it had (a Born pass runs the
    forward body, which is also what accumulates the pseudo-Hessian when it is armed)."""
    from sepfwi import _native
    pb, v, _ = prob_a
    hip_ops.release()
    fn = pb["para_fname"]
    m = [t.cuda() for t in pb["lame_init"]]
    tv = [torch.from_numpy(a).cuda() for a in v]
    hip_ops.obscalc(*[t.cuda() for t in pb["lame_true"]], pb["Stf"], 1, pb["Shot_ids"], fn, to_store=True)
    out = hip_ops.backward(*m, pb["Stf"], 1, pb["Shot_ids"], fn, pseudo_hessian=2)
    before = [h.cpu() for h in out[5:8]]
    assert len(before) == 3 and all(h.abs().max() > 0 for h in before)

    def read():
        H = torch.empty((3,) + tuple(m[0].shape), dtype=torch.float32)
        _native.check(_native.lib().sepfwi_get_pseudo_hessian(fn.encode(), 0, *[C.c_void_p(H[k].data_ptr()) for k in range(3)]))
        return H

    assert all(torch.equal(a, b) for a, b in zip(read(), before))
    hip_ops.born(*m, *tv, pb["Stf"], 1, pb["Shot_ids"], fn, components=COMPS)
    assert all(torch.equal(a, b) for a, b in zip(read(), before)), "after the Born call"
    hip_ops.gauss_newton(*m, *tv, pb["Stf"], 1, pb["Shot_ids"], fn)
    assert all(torch.equal(a, b) for a, b in zip(read(), before)), "after the product"
    again = hip_ops.backward(*m, pb["Stf"], 1, pb["Shot_ids"], fn, pseudo_hessian=2)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(again[5:8], before)) and all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(again[:4], out[:4]))


def test_gauss_newton_product_with_img_every_2(hip_ops, prob_a):
    """5: img_every = 2 (the imaging condition on every second step) -- the product is the gradient `backward` returns at shifted data
    under the same option, and not the one of img_every = 1."""
    pb, v, _ = prob_a
    hip_ops.release()
    m = [t.cuda() for t in pb["lame_init"]]
    tv = [torch.from_numpy(a).cuda() for a in v]
    every = [t.cpu().numpy() for t in hip_ops.gauss_newton(*m, *tv, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])]
    with P.kernel_options(img_every=2):
        dev, bound, _ = gn_against_backward(hip_ops, pb, v, (1.0, 0.0, 0.0), "img2")
        second = [t.cpu().numpy() for t in hip_ops.gauss_newton(*m, *tv, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])]
    assert max(dev) <= bound, (dev, bound)
    assert all(not np.array_equal(a, b) for a, b in zip(second, every)), "img_every = 2 changed nothing: the option was not in force"
    hip_ops.release()


def test_quiet_skip_is_ignored_by_born_calls_after_a_quiet_misfit_call(hip_ops, prob_a):
    """quiet_skip = 1: a plain misfit call on the fused channel line leaves quiet maps in the session (quiet_total > 0).  Born
    modelling and the product of the SAME session under the same option then ignore the option -- the scattered field has no quiet
    maps, and the product's backward half must not consult stale or empty ones: gathers and hv equal, bit for bit, those of a fresh
    session that never saw the option."""
    pb, v, _ = prob_a
    fn, _ = write_para(pb, "quiet")
    m = [t.cuda() for t in pb["lame_init"]]
    tv = [torch.from_numpy(a).cuda() for a in v]
    hip_ops.release()
    with P.kernel_options(quiet_skip=1):
        hip_ops.obscalc(*[t.cuda() for t in pb["lame_true"]], pb["Stf"], 1, pb["Shot_ids"], fn, to_store=True)
        hip_ops.forward(*m, pb["Stf"], 0, pb["Shot_ids"], fn)
        assert hip_ops.stats(fn)["quiet_total"] > 0, "the misfit call did not run with quiet maps: the test would compare nothing"
        quiet = gpu_born(hip_ops, pb, v, para_fname=fn)
        hv_quiet = [t.cpu() for t in hip_ops.gauss_newton(*m, *tv, pb["Stf"], 1, pb["Shot_ids"], fn)]
    hip_ops.release()
    with P.kernel_options(quiet_skip=0):
        plain = gpu_born(hip_ops, pb, v, para_fname=fn)
        hv_plain = [t.cpu() for t in hip_ops.gauss_newton(*m, *tv, pb["Stf"], 1, pb["Shot_ids"], fn)]
    for c in COMPS:
        assert np.abs(plain[c]).max() > 0 and np.array_equal(quiet[c], plain[c]), c
    for k in range(3):
        assert hv_plain[k].abs().max() > 0 and torch.equal(hv_quiet[k], hv_plain[k]), "hv %d" % k
    hip_ops.release()
