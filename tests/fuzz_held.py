"""What the GPU fuzz tests of the misfit kinds share around their comparisons (tests/test_gpu_envelope_fuzz.py,
tests/test_gpu_robust_fuzz.py): the flat layout of the data-space entries and the two comparisons that print before they judge.  cond: the
misfit's own conditioning term (fuzz_sides.cond_env, fuzz_sides.cond_robust), printed under `name`."""
import numpy as np
import torch

import fuzz_common as C


def flat(gathers):
    return torch.from_numpy(np.concatenate([np.asarray(g, np.float32).reshape(-1) for g in gathers]))


def unflat(t, like):
    a, out, off = t.cpu().numpy(), [], 0
    for g in like:
        out.append(a[off:off + g.size].reshape(g.shape))
        off += g.size
    return out


def held(bad, got, ref, alt, what, nominal, cond, scale=None, name="cond_env"):
    """fuzz_common.scalar_held with the conditioning term; prints the deviation, a miss goes to `bad`"""
    scale = abs(ref) if scale is None else scale
    print("%s: got %.8e, reference %.8e, deviation %.2e of the scale (the two oracle builds %.2e, %s %.1e)"
          % (what, got, ref, abs(got - ref) / max(scale, 1e-300), abs(alt - ref) / max(scale, 1e-300), name, cond))
    if not C.scalar_held(got, ref, alt, nominal, scale, cond):
        bad.append(what)


def gathers_held(bad, got, ref, alt, what, cond, name="cond_env"):
    """per gather, rel-L2: |got - ref| <= (1e-4 + cond) |ref| + 3 |alt - ref|; prints the deviation, a miss goes to `bad`.  The
    gather of a shot whose wave has not reached its channels is the stencil's precursor (seed 10, shots 0, 1 and 3: 1e-14 and below),
    and what the misfit makes of it -- its third power -- lies in float32's subnormal range or is 0: where 1e-4 of the reference's
    maximum is below the spacing of the numbers both sides must stay subnormal, and nothing else can be asked
    (tests/test_gpu_conditioned_gn_fuzz.py: against_the_oracle)."""
    tiny = float(np.finfo(np.float32).tiny)
    for i, (g, r, a) in enumerate(zip(got, ref, alt)):
        top = float(np.abs(r).max())
        if C.GATHER_TOL * top < tiny:
            print("%s, gather %d: the reference's maximum is %.1e, below float32's normal range; the GPU's %.1e" % (what, i, top, float(np.abs(g).max())))
            if not float(np.abs(g).max()) < tiny / C.GATHER_TOL:
                bad.append("%s, gather %d" % (what, i))
            continue
        print("%s, gather %d (%d channels): rel-L2 %.2e (the two oracle builds' C on the same gathers %.2e, %s %.1e)"
              % (what, i, r.shape[0], C.rel(C.d64(g, r), r), C.rel(C.d64(a, r), r), name, cond))
        if not (np.isfinite(g).all() and C.array_held(g, r, a, C.GATHER_TOL, cond)):
            bad.append("%s, gather %d" % (what, i))
