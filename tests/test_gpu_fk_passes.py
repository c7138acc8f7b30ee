"""The fan filter inside the passes on the GPU (-m gpu): misfit and gradient calls, the exact gradient and the exact Gauss-Newton product under
a parameter file with if_win, filter and fk_slowness (fk_ref.pass_problem: cond_gn_ref.SMALL -- 40 x 48, 120 steps, 2 shots of 40 channels --
in mode "both" plus the fan), observed data installed through the store.  C is tests/fk_ref.py's (the oracle's window and band-pass, then
the float64 fan), J tests/born_ref.py's; tests/test_fk_reference.py shows on the CPU that every J v and residual used here changes by more
than 10 % in norm through the fan.

Tolerances, none new:
  1     the misfit of calc_id 0 and 1 against data_misfit of the library's own raw gathers: 2^-23 relative (the same kernels on the same
        bits; the sum over the traces is the one double addition whose order may differ)
  2, 3  tests/test_gpu_conditioned_gauss_newton.py's: |got - ref| <= 1e-3 scale + 3 |alt - ref| (exact_adjoint_ref.held; alt: the nvfma build)
  4     sepfwi_stats.launches: an exact count, 2 x 9 per shot with channels (csrc/conditioning.hpp: launches())
  5     bit for bit
Every comparison prints its deviation before it asserts; profiles/r32_fk_filter.txt holds the figures measured on the MI355X.

On the parent commit the library ignores the keys: 2 and 3 fail on the missing fan (the inputs discriminate), 4 counts no stage."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cond_gn_ref as G
import exact_adjoint_ref as X
import fk_ref as F
import problems as P
from exact_adjoint_ref import cuda, held
from sepfwi import utils as ft

pytestmark = pytest.mark.gpu
V_SEEDS = (3, 4)
FK_LAUNCHES = 9      # embed, R2C, transposition, C2C, the gain, C2C, transposition, C2R, crop (csrc/conditioning.hpp)


def model(pb, which="lame_init"):
    return [t.cuda() for t in pb[which]]


def flat(gathers):
    return torch.from_numpy(np.concatenate([np.asarray(g, np.float32).reshape(-1) for g in gathers]))


class Side:
    """the problem and its reference quantities on both oracle builds: Z C J v per v, the raw gathers, Z (C obs - C syn)"""

    def __init__(self, oracle, oracle_nvfma, tmp):
        self.pb = pb = F.pass_problem(tmp)
        self.libs = (oracle, oracle_nvfma)
        self.vs = [X.smooth_v(pb, s) for s in V_SEEDS]
        self.zcjv = [[[G.Z(c) for c in G.C_all(lib, pb, G.jv_ett(lib, pb, v), F.C_of)] for v in self.vs] for lib in self.libs]      # [build][v][shot]
        self.obs, self.res = [], []
        for lib in self.libs:
            obs, _ = G.oracle_gathers(lib, pb, "lame_true")
            syn, _ = G.oracle_gathers(lib, pb, "lame_init")
            self.obs.append(obs)
            self.res.append([G.Z(np.asarray(F.C_of(lib, pb, o, s), np.float64) - F.C_of(lib, pb, y, s)) for o, y, s in zip(obs, syn, G.shots_of(pb))])

    def install(self, hip_ops, pb=None):
        pb = pb or self.pb
        for i, sid in enumerate(G.shots_of(pb)):
            hip_ops.set_observed(pb["para_fname"], sid, torch.from_numpy(np.ascontiguousarray(self.obs[0][i])))

    def norm2(self, k, b=0):
        return G.dot(self.zcjv[b][k], self.zcjv[b][k])

    def cross(self, j, k, b=0):
        return G.dot(self.zcjv[b][j], self.zcjv[b][k])


@pytest.fixture(scope="module")
def side(oracle, oracle_nvfma, hip_ops, tmp_path_factory):
    """computed once, left unchanged"""
    return Side(oracle, oracle_nvfma, tmp_path_factory.mktemp("fk_passes"))


# ---- 1: the misfit of a call ------------------------------------------------------------------------------------------------------------------
def test_misfit_of_a_call_equals_data_misfit_of_its_own_gathers(hip_ops, side):
    pb = side.pb
    hip_ops.release()
    raw = F.without_fk(G.set_mode(pb, "none", name="raw_keys"), name="raw")      # no conditioning key at all: the library's raw gathers
    hip_ops.obscalc(*model(pb), pb["Stf"], 1, raw["Shot_ids"], raw["para_fname"])
    syn = [np.ascontiguousarray(ft.read_shot_gather(raw["para"]["data_dir_name"], "ett", sid, pb["nSteps"])) for sid in G.shots_of(pb)]
    fd, _ = hip_ops.data_misfit(flat(side.obs[0]).cuda(), flat(syn).cuda(), pb["Shot_ids"], pb["para_fname"])
    hip_ops.release()
    side.install(hip_ops)
    f0 = float(hip_ops.forward(*model(pb), pb["Stf"], 0, pb["Shot_ids"], pb["para_fname"])[0])
    f1 = float(hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])[0])
    ref = 0.5 * G.dot(side.res[0], side.res[0])
    print("fk passes 1: calc_id 0 %.8e, calc_id 1 %.8e, data_misfit of the library's own gathers %.8e (gaps %.2e and %.2e, bound 2^-23 = %.2e); "
          "the reference's at the oracle's gathers %.8e (%.2e)" % (f0, f1, fd, abs(f0 - fd) / fd, abs(f1 - fd) / fd, 2.0 ** -23, ref, abs(fd - ref) / ref))
    assert fd > 0 and abs(f0 - fd) <= 2.0 ** -23 * fd and abs(f1 - fd) <= 2.0 ** -23 * fd
    hip_ops.release()


# ---- 2: the exact product -------------------------------------------------------------------------------------------------------------------------
def test_exact_product_is_symmetric_and_equals_the_norm_of_zcjv(hip_ops, side):
    """v^T H v = |Z C J v|^2 for two smooth v on Omega; u^T H v = v^T H u, and both = <Z C J u, Z C J v>"""
    pb = side.pb
    hip_ops.release()
    hv = [[h.cpu().numpy() for h in hip_ops.gauss_newton(*model(pb), *cuda(v), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact=True)] for v in side.vs]
    vhv = [X.model_dot(v, h) for v, h in zip(side.vs, hv)]
    for k in range(2):
        X.outside_is_zero(pb, hv[k], "fk passes 2")
        held(vhv[k], side.norm2(k), side.norm2(k, 1), "fk passes 2 v^T H v, v %d" % k)
    scale = float(np.sqrt(vhv[0] * vhv[1]))
    c21, c12 = X.model_dot(side.vs[1], hv[0]), X.model_dot(side.vs[0], hv[1])
    cr, ca = side.cross(0, 1), side.cross(0, 1, 1)
    held(c21, c12, c12 + (ca - cr), "fk passes 2 symmetry <u, H v> against <v, H u>", scale=scale)
    held(c21, cr, ca, "fk passes 2 <u, H v> against <Z C J u, Z C J v>", scale=scale)
    hip_ops.release()


# ---- 3: the exact gradient ------------------------------------------------------------------------------------------------------------------------
def test_exact_gradient_of_the_conditioned_misfit(hip_ops, side):
    """<g, v> = -<Z C J v, Z (C obs - C syn)>"""
    pb = side.pb
    hip_ops.release()
    side.install(hip_ops)
    out = hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact_adjoint=True)
    g = [t.cpu().numpy() for t in out[1:4]]
    X.outside_is_zero(pb, g, "fk passes 3")
    mis = [0.5 * G.dot(r, r) for r in side.res]
    f = float(out[0])
    print("fk passes 3: misfit of the exact pass %.8e, of the reference %.8e (relative gap %.2e; the two oracle builds %.2e)" % (f, mis[0], abs(f - mis[0]) / mis[0], abs(mis[1] - mis[0]) / mis[0]))
    assert abs(f - mis[0]) <= 1e-4 * mis[0] + 3.0 * abs(mis[1] - mis[0])
    for k in range(2):
        rr, aa = -G.dot(side.zcjv[0][k], side.res[0]), -G.dot(side.zcjv[1][k], side.res[1])
        cosine = rr / np.sqrt(side.norm2(k) * G.dot(side.res[0], side.res[0]))
        held(X.model_dot(side.vs[k], g), rr, aa, "fk passes 3 <g, v>, v %d (cosine %.3f)" % (k, cosine), scale=abs(rr))
    hip_ops.release()


# ---- 4: the launches ------------------------------------------------------------------------------------------------------------------------------
def test_gradient_call_counts_the_stage(hip_ops, side):
    """a gradient call under the file against the same file without the fk keys: C and C^T once each per shot with channels"""
    def launches_of(pb):
        hip_ops.release()
        with P.kernel_options(batch=0):
            side.install(hip_ops, pb)
            hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
            n = hip_ops.stats(pb["para_fname"])["launches"]
        hip_ops.release()
        return n
    pb = side.pb
    shots = sum(1 for s in G.shots_of(pb) if int(pb["survey"]["shot%d" % s]["nrec"]) > 0)
    got = launches_of(pb) - launches_of(F.without_fk(pb, "count_nofk"))
    print("fk passes 4: launches with the fk keys - without = %d; 2 x %d x %d shots = %d" % (got, FK_LAUNCHES, shots, 2 * FK_LAUNCHES * shots))
    assert got == 2 * FK_LAUNCHES * shots


# ---- 5: a file without the keys ---------------------------------------------------------------------------------------------------------------------
CHILD = """
import sys
import numpy as np, torch
from sepfwi import fwi_ops
z = np.load(sys.argv[1])
m = [torch.from_numpy(z[k]).cuda() for k in ("lam", "mu", "den")]
for i, sid in enumerate(z["ids"].tolist()):
    fwi_ops.set_observed(sys.argv[2], sid, torch.from_numpy(z["obs%d" % i]))
out = fwi_ops.backward(*m, torch.from_numpy(z["stf"]), 1, torch.from_numpy(z["ids"]), sys.argv[2])
np.savez(sys.argv[3], **{"o%d" % i: t.cpu().numpy() for i, t in enumerate(out)})
"""


def test_a_file_without_the_keys_gives_the_bits_of_a_process_that_never_saw_them(hip_ops, side, tmp_path):
    """this process has run the fan (and does so again first); a fresh process runs the file without the keys alone"""
    from conftest import ROOT
    pb = side.pb
    nofk = F.without_fk(pb, "bits_nofk")
    hip_ops.release()
    side.install(hip_ops)
    with_fk = hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    side.install(hip_ops, nofk)
    here = [t.cpu().numpy() for t in hip_ops.backward(*model(pb), pb["Stf"], 1, nofk["Shot_ids"], nofk["para_fname"])]
    assert float(with_fk[0]) != float(here[0])
    args = str(tmp_path / "in.npz"), nofk["para_fname"], str(tmp_path / "out.npz")
    np.savez(args[0], lam=pb["lame_init"][0].numpy(), mu=pb["lame_init"][1].numpy(), den=pb["lame_init"][2].numpy(), stf=pb["Stf"].numpy(),
             ids=pb["Shot_ids"].numpy(), **{"obs%d" % i: np.ascontiguousarray(o) for i, o in enumerate(side.obs[0])})
    hip_ops.release()
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "sep-2023_amd")] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    subprocess.run([sys.executable, "-c", CHILD, *args], env=env, check=True, timeout=300)
    there = np.load(args[2])
    for i, a in enumerate(here):
        assert np.array_equal(a, there["o%d" % i]), "output %d of the file without the keys differs from a fresh process's" % i
    assert all(np.abs(a).max() > 0 for a in here[:4])
