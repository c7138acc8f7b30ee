"""The diagonal pseudo-Hessian on the GPU (-m gpu): csrc/pseudo_hessian.hip through sepfwi_pseudo_hessian_arm / sepfwi_get_pseudo_hessian
and fwi_ops.backward / forward(pseudo_hessian=k), against the float64 restatement over the CPU oracle (tests/pseudo_hessian_ref.py).

Tolerance against the reference, per array: max-norm deviation <= 1e-4 of the array's maximum and rel-L2 <= 1e-4.  The kernels
accumulate in float32 where the reference accumulates in float64; a float32 accumulation of the same terms deviates by at most 3.8e-6
of the maximum (rel-L2 1.9e-6) on these problems, so 1e-4 leaves a factor 25 for another order of operations and is far below the
1e-3 the suite allows gradients -- an error in a stencil tap, a constant or the placement in the step is >= 1e-2."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import problems as P
import pseudo_hessian_ref as R
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
TOL = 1e-4
NAMES = ("hLambda", "hMu", "hDen")
B4 = dict(R.PROBLEM_B, nshots=4)      # four shots on three forward lanes: a lane is used twice


def _setup(workdir, kw, hip_ops):
    """A problem whose session holds the observed data of the true model (no files)."""
    pb = P.make_problem(str(workdir), **kw)
    hip_ops.obscalc(*pb["lame_true"], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], to_store=True)
    return pb


def _reference(oracle, pb, every):
    return R.pseudo_hessian(oracle, *[t.numpy() for t in pb["lame_init"]], pb["Stf"].numpy(), pb["Shot_ids"].numpy(), pb["para"], pb["survey"],
                            every=every)[0]


@pytest.fixture(scope="module")
def prob_a(oracle, hip_ops, tmp_path_factory):
    pb = _setup(tmp_path_factory.mktemp("ph_a"), R.PROBLEM_A, hip_ops)
    return pb, _reference(oracle, pb, (1,))


@pytest.fixture(scope="module")
def prob_b(oracle, hip_ops, tmp_path_factory):
    pb = _setup(tmp_path_factory.mktemp("ph_b"), B4, hip_ops)
    return pb, _reference(oracle, pb, (1, 3, 4))


def _armed(hip_ops, pb, every=1, ids=None, ngpu=1, calc="backward", models=None):
    lam, mu, den = models or pb["lame_init"]
    ids = pb["Shot_ids"] if ids is None else torch.as_tensor(ids, dtype=torch.int32)
    if calc == "forward":
        out = hip_ops.forward(lam, mu, den, pb["Stf"], 0, ids, pb["para_fname"], pseudo_hessian=every)
        return out[:1], [h.cpu().numpy().copy() for h in out[1:]]
    out = hip_ops.backward(lam, mu, den, pb["Stf"], ngpu, ids, pb["para_fname"], pseudo_hessian=every)
    assert len(out) == 8
    return out[:5], [h.cpu().numpy().copy() for h in out[5:]]


def _plain(hip_ops, pb):
    return hip_ops.backward(*pb["lame_init"], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])


def _close(got, want, what):
    worst = []
    for name, g, w in zip(NAMES, got, want):
        w = np.asarray(w, np.float64)
        assert g.shape == w.shape and np.isfinite(g).all() and w.max() > 0, (what, name)
        dmax, l2 = np.abs(g - w).max() / w.max(), P.rel_l2(g, w)
        worst.append((dmax, l2))
        print("pseudo-Hessian %s, %s: max-norm deviation %.2e of the maximum, rel-L2 %.2e" % (what, name, dmax, l2))
    for name, (dmax, l2) in zip(NAMES, worst):
        assert dmax <= TOL and l2 <= TOL, (what, name, dmax, l2)


def _same_bits(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        assert np.array_equal(x, y), (what, name, float(np.abs(x - y).max()))


def test_batched_schedule_matches_the_reference(hip_ops, prob_a):
    """1: batch = 1, 50 x 90, two shots (k_pseudo_hessian_batch, one accumulator set per sub-batch stream), gradient call, every step."""
    pb, ref = prob_a
    with P.kernel_options(batch=1):
        _, H = _armed(hip_ops, pb)
    _close(H, ref[1], "batched 50x90")
    inside = np.asarray(ref[1][0]) > 0
    for name, h in zip(NAMES, H):
        assert (h[~inside] == 0).all() and (h[inside] > 0).all(), name      # zero outside the interior, illuminated inside


def test_batched_schedule_with_two_shots_per_sub_batch_matches_the_reference(hip_ops, prob_b):
    """1b: four shots as two sub-batches of two: the wave's loop over the shots of its sub-batch, one read-modify-write per step."""
    pb, ref = prob_b
    with P.kernel_options(batch=1):
        _, H = _armed(hip_ops, pb)
        launches = hip_ops.stats(pb["para_fname"], 0)["launches"]
        _plain(hip_ops, pb)
        assert launches == hip_ops.stats(pb["para_fname"], 0)["launches"] + 2 * (pb["nSteps"] - 1) + 1      # two launches per step for four shots
    _close(H, ref[1], "batched 40x150, 2 + 2 shots")


@pytest.mark.parametrize("every", [1, 3])
def test_stream_schedule_with_reused_lanes_matches_the_reference(hip_ops, prob_b, every):
    """2: batch = 0, 40 x 150 x 400 steps, four shots on three lanes (k_pseudo_hessian, one accumulator set per lane), each stride
    against the reference evaluated with the same stride."""
    pb, ref = prob_b
    with P.kernel_options(batch=0):
        _, H = _armed(hip_ops, pb, every=every)
    _close(H, ref[every], "streams 40x150 every %d" % every)


def test_time_stride_on_the_gpu_is_recorded(hip_ops, prob_b):
    """every = 4 against every = 1 on the GPU: a quadrature of the same time integral.  The reference pair differs by up to 7.7e-4
    rel-L2 (rho) on these problems -- too close to 1e-3 to assert, so the GPU pair must only differ as the reference pair does."""
    pb, ref = prob_b
    with P.kernel_options(batch=0):
        H1, H4 = _armed(hip_ops, pb, every=1)[1], _armed(hip_ops, pb, every=4)[1]
    for name, a, b, ra, rb in zip(NAMES, H4, H1, ref[4], ref[1]):
        got, want = P.rel_l2(a, b), P.rel_l2(ra, rb)
        print("pseudo-Hessian every = 4 against every = 1, %s: GPU rel-L2 %.2e, reference %.2e" % (name, got, want))
        assert abs(got - want) <= 2 * TOL, name
    _close(H4, ref[4], "streams 40x150 every 4")


@pytest.mark.parametrize("batch", [0, 1])
def test_misfit_call_and_gradient_call_give_the_same_bits(hip_ops, prob_a, batch):
    """3: the forward passes of calc_id 0 and 1 are the same launches in the same order."""
    pb, _ = prob_a
    with P.kernel_options(batch=batch):
        (m0,), Hf = _armed(hip_ops, pb, calc="forward")
        out, Hb = _armed(hip_ops, pb)
    _same_bits(Hf, Hb, "forward vs backward, batch %d" % batch)
    assert float(m0) == float(out[0])


@pytest.mark.parametrize("batch", [0, 1])
def test_arming_leaves_results_and_disarmed_launches_alone(hip_ops, prob_a, tmp_path, batch):
    """4: misfit, gradients and gStf of an armed call are those of a disarmed one, bit for bit; the armed call issues exactly one more
    launch per shot (sub-batch) and accumulating step plus the finalisation; after disarming, a call issues the launches of a session
    that was never armed."""
    pb, _ = prob_a
    fresh = _setup(tmp_path, R.PROBLEM_A, hip_ops)      # same problem, a session of its own, never armed
    with P.kernel_options(batch=batch):
        _plain(hip_ops, fresh)
        _plain(hip_ops, fresh)
        never = hip_ops.stats(fresh["para_fname"], 0)["launches"]
        plain = [t.cpu().numpy().copy() for t in _plain(hip_ops, pb)]
        out, H = _armed(hip_ops, pb)
        armed = hip_ops.stats(pb["para_fname"], 0)["launches"]
        again = [t.cpu().numpy().copy() for t in _plain(hip_ops, pb)]
        after = hip_ops.stats(pb["para_fname"], 0)["launches"]
    for k in range(5):
        assert np.array_equal(out[k].cpu().numpy(), plain[k]) and np.array_equal(again[k], plain[k]), k
    assert after == never
    per_step = pb["Shot_ids"].numel()      # two shots: a lane each (streams), a sub-batch stream each (batched, option batch_split = 2)
    assert armed == after + per_step * (pb["nSteps"] - 1) + 1


@pytest.mark.parametrize("batch", [0, 1])
def test_two_armed_calls_give_the_same_bits(hip_ops, prob_a, batch):
    """5: no atomics, and the accumulators are zeroed at the start of every armed call."""
    pb, _ = prob_a
    with P.kernel_options(batch=batch):
        _same_bits(_armed(hip_ops, pb)[1], _armed(hip_ops, pb)[1], "repeat, batch %d" % batch)


@pytest.mark.parametrize("batch", [0, 1])
def test_shots_add_up(hip_ops, prob_a, batch):
    """6: H(shots {0, 1}) = H({0}) + H({1}) within the tolerance of test 1."""
    pb, _ = prob_a
    with P.kernel_options(batch=batch):
        both, h0, h1 = _armed(hip_ops, pb)[1], _armed(hip_ops, pb, ids=[0])[1], _armed(hip_ops, pb, ids=[1])[1]
    for a, b in zip(h0, h1):
        assert a.max() > 0 and b.max() > 0 and not np.array_equal(a, b)
    _close(both, [a.astype(np.float64) + b for a, b in zip(h0, h1)], "additivity, batch %d" % batch)


def test_quiet_segments_change_no_bit(hip_ops, prob_a):
    """7: the fields of a skipped row segment are the +0 they would hold anyway."""
    pb, _ = prob_a
    with P.kernel_options(batch=0, quiet_skip=0):
        off = _armed(hip_ops, pb)[1]
    with P.kernel_options(batch=0, quiet_skip=1):
        on = _armed(hip_ops, pb)[1]
        assert hip_ops.stats(pb["para_fname"], 0)["quiet_total"] > 0      # the option was live for this shot geometry
    _same_bits(on, off, "quiet_skip")


def test_armed_gradient_call_keeps_the_persistent_loop(hip_ops, tmp_path):
    """8: the accumulation is a forward-pass matter -- on a loop-sized grid the backward pass of an armed call still runs as the ONE
    persistent launch, and its gradients are those of the disarmed call, bit for bit."""
    pb = _setup(tmp_path, dict(nz=300, nx=500, nPml=10, nSteps=140, nshots=1, hetero=True, rec_z=40), hip_ops)
    with P.kernel_options(batch=0, bwd_fuse=4):
        plain = [t.cpu().numpy().copy() for t in _plain(hip_ops, pb)]
        assert hip_ops.stats(pb["para_fname"], 0)["persist_steps"] == pb["nSteps"] - 1, hip_ops.loop_status(pb["para_fname"])
        out, H = _armed(hip_ops, pb)
        assert hip_ops.stats(pb["para_fname"], 0)["persist_steps"] == pb["nSteps"] - 1, hip_ops.loop_status(pb["para_fname"])
    for k in range(5):
        assert np.array_equal(out[k].cpu().numpy(), plain[k]), k
    assert all(np.isfinite(h).all() and h.max() > 0 for h in H)


def test_errors_null_outputs_and_rearming(hip_ops, tmp_path):
    """9: through the C ABI."""
    from sepfwi import _native
    L = _native.lib()
    pb = _setup(tmp_path, R.PROBLEM_A, hip_ops)
    fn = pb["para_fname"].encode()
    shape = (pb["nz_pad"], pb["nx_pad"])
    new = lambda: np.full(shape, -1.0, np.float32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    with P.kernel_options(batch=0):
        _plain(hip_ops, pb)
        a = new()
        assert L.sepfwi_get_pseudo_hessian(fn, 0, ptr(a), None, None) == -1 and b"no armed call yet" in L.sepfwi_last_error()
        assert (a == -1.0).all()
        assert L.sepfwi_pseudo_hessian_arm(fn, 0, -2) == -1
        try:
            assert L.sepfwi_pseudo_hessian_arm(fn, 0, 1) == 0
            _plain(hip_ops, pb)                                   # (armed through the C ABI: the operator call itself is the plain one)
            h1 = [new() for _ in range(3)]
            assert L.sepfwi_get_pseudo_hessian(fn, 0, *[ptr(h) for h in h1]) == 0
            only_mu = new()
            assert L.sepfwi_get_pseudo_hessian(fn, 0, None, ptr(only_mu), None) == 0      # NULL outputs are skipped
            assert np.array_equal(only_mu, h1[1])
            assert L.sepfwi_get_pseudo_hessian(fn, 0, None, None, None) == 0
            dev = torch.full(shape, -1.0, dtype=torch.float32, device="cuda")              # a device pointer
            assert L.sepfwi_get_pseudo_hessian(fn, 0, None, None, C.c_void_p(dev.data_ptr())) == 0
            assert np.array_equal(dev.cpu().numpy(), h1[2])
            assert L.sepfwi_pseudo_hessian_arm(fn, 0, 3) == 0     # another stride: from the next call on
            again = [new() for _ in range(3)]
            assert L.sepfwi_get_pseudo_hessian(fn, 0, *[ptr(h) for h in again]) == 0
            _same_bits(again, h1, "re-armed, no call yet")
            _plain(hip_ops, pb)
            h3 = [new() for _ in range(3)]
            assert L.sepfwi_get_pseudo_hessian(fn, 0, *[ptr(h) for h in h3]) == 0
        finally:
            assert L.sepfwi_pseudo_hessian_arm(fn, 0, 0) == 0
        hip_ops.obscalc(*pb["lame_true"], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], to_store=True)     # calc_id 3 never accumulates
        kept = [new() for _ in range(3)]
        assert L.sepfwi_get_pseudo_hessian(fn, 0, *[ptr(h) for h in kept]) == 0
        _same_bits(kept, h3, "after disarming")
        _same_bits(_armed(hip_ops, pb, every=1)[1], h1, "operator every 1 vs C ABI")
        _same_bits(_armed(hip_ops, pb, every=3)[1], h3, "operator every 3 vs C ABI")
    assert not np.array_equal(h1[0], h3[0])


def test_thread_path_ngpu2_pinned_to_one_gpu(hip_ops, prob_b):
    """10a: single-process ngpu = 2, both threads on the one card (they share ONE session and take turns): the parts are summed like
    the gradients."""
    pb, ref = prob_b
    with P.kernel_options(batch=0):
        one = _armed(hip_ops, pb)[1]
        hip_ops.device_override = 0
        try:
            out, two = _armed(hip_ops, pb, ngpu=2)
            dev = [t.cuda() for t in pb["lame_init"]]
            out_d, two_d = _armed(hip_ops, pb, ngpu=2, models=dev)
        finally:
            hip_ops.device_override = None
    _close(two, [h.astype(np.float64) for h in one], "ngpu 2 on one card vs ngpu 1")
    _close(two, ref[1], "ngpu 2 on one card vs reference")
    _same_bits(two_d, two, "device-resident model")


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, workdir, q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "sep-2023_amd"), os.path.join(ROOT, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as td
    td.init_process_group("gloo", rank=rank, world_size=world)
    import problems as P2
    import pseudo_hessian_ref as R2
    from sepfwi import dist, fwi_ops
    fwi_ops.device_override = 0
    pb = P2.make_problem(os.path.join(workdir, "rank%d" % rank), **R2.PROBLEM_B)
    para = dict(pb["para"]); para["data_dir_name"] = os.path.join(workdir, "Data")      # the observed data the parent wrote
    json.dump(para, open(pb["para_fname"], "w"))
    lam, mu, den = [t.cuda() for t in pb["lame_init"]]
    out = fwi_ops.backward(lam, mu, den, pb["Stf"], world, pb["Shot_ids"], pb["para_fname"], pseudo_hessian=1)
    q.put((rank, float(out[0]), [t.cpu().numpy() for t in out[1:4]], [t.cpu().numpy() for t in out[5:8]], dist.collective_stats()["calls"]))
    td.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_gloo_ranks_on_one_gpu_match_single_process(hip_ops, tmp_path):
    """10b: under torch.distributed every rank ends with the H of all shots -- one more all-reduce, of the fused [hL | hM | hD] buffer;
    the gradient collective is the one it was."""
    work = str(tmp_path)
    pb = P.make_problem(os.path.join(work, "single"), **R.PROBLEM_B)
    para = dict(pb["para"]); para["data_dir_name"] = os.path.join(work, "Data")
    json.dump(para, open(pb["para_fname"], "w"))
    os.makedirs(para["data_dir_name"], exist_ok=True)
    hip_ops.obscalc(*pb["lame_true"], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    ref, H = _armed(hip_ops, pb)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, work, q)) for r in range(2)]
    [p.start() for p in procs]
    res = sorted([q.get(timeout=240) for _ in range(2)], key=lambda t: t[0])
    [p.join(60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    for r in res:
        assert abs(r[1] - float(ref[0])) <= 1e-5 * abs(float(ref[0]))
        for k in range(3):
            assert P.rel_l2(r[2][k], ref[k + 1].cpu().numpy()) <= 1e-5
        _close(r[3], [h.astype(np.float64) for h in H], "gloo rank %d vs one process" % r[0])
        assert r[4] == 1                                          # the gradient collective's record: still one call
    _same_bits(res[0][3], res[1][3], "rank 0 vs rank 1")


def _run_example(extra, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "fwi_anomaly_vp_vs_den.py"), "--device", "cuda", "--workdir", str(tmp_path)] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=500, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, out.stderr[-2000:]
    its = [ln for ln in out.stdout.splitlines() if ln.startswith("iterate ")]
    return [float(ln.split("misfit")[1].split()[0]) for ln in its], out.stdout


@pytest.mark.timeout(600)
def test_example_with_the_preconditioner_reduces_the_misfit(tmp_path):
    """11a: examples/fwi_anomaly_vp_vs_den.py --precond 1e-3, three iterations."""
    f, text = _run_example(["--niter", "3", "--precond", "1e-3"], tmp_path)
    print(text)
    assert "preconditioner: scale" in text and len(f) >= 2
    assert f[-1] < f[0]


@pytest.mark.timeout(600)
def test_example_without_the_flag_prints_the_iterates_it_printed(tmp_path):
    """11b: without --precond the example is the reference's experiment 001: iterates 0, 1, 2 are those of the reference's printed log
    (tests/golden/known_answers.json) at the bounds tests/test_known_answers.py holds the HIP path to (1e-4, 5e-4, 1e-3)."""
    f, text = _run_example(["--niter", "2"], tmp_path)
    assert "preconditioner" not in text and len(f) == 3, text
    want = json.load(open(os.path.join(GOLDEN, "known_answers.json")))["001"]["lbfgs_f"]
    for k, tol in enumerate((1e-4, 5e-4, 1e-3)):
        assert abs(f[k] - want[k]) <= tol * want[k], (k, f[k], want[k])
