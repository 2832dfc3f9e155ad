"""The Floor0 kernels (floor0.hip: floor0_apply_kernel, floor0_wtab_kernel, floor0_curve_kernel; synth_dual.hip:
floor0_multiply_x2) at the limits of order, bark map and grid, against the CPU oracle (oracle.floor0_apply through
helpers.oracle_decode) at the bar of test_floor0_matches_oracle: |got - ref|max <= 1e-5 * max(1, |ref|max).  The cases are
floor0_cases.CASES; test_floor0_cases_cpu.py shows with the oracle alone that each of them would notice a wrong index.
  A  orders 1 ... 255 in every order % 4 class below and above the 64-coefficient prefetch, four coefficient strides, two
     type-0 floors of orders 65 and 7 swapped by block size, silence by the amplitude's sign;
  B  bark maps of 1 ... 1024 entries (one to four rounds of 256 indices, whole and partial), orders 16 and 65;
  C  floor0_apply_kernel where it has no fused twin: mono, three channels with floors [0, 1, 0], 4096 blocks with bark maps beyond
     kFloor0MaxBark in front of the big kernel, the any-size path;
  D  8400 records in one call: wavefronts of the persistent grid take a second record.
Every case: about 12 frames (D: 4208) in two synth calls with the state carried across them, one silent type-0 record.  Where the
stereo fast path takes the setup (A, B, D) the fused run and the VPZ_NO_F0_FUSED=1 run are the same bits, and both meet the bar.
Bark maps larger than half a block have no reference -- the oracle refuses them, as the reference throws -- and stay out of scope."""
import numpy as np
import pytest

import floor0_cases as fc
from gpu_context import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def decode(ctx, b, fused, capfd):
    """The case's calls on one decoder; fused False: VPZ_NO_F0_FUSED=1, planar temp + floor0_apply_kernel.  Returns the PCM and
    the routes the calls took, as VPZ_HOST_PROFILE=1 names them."""
    import re
    from synth_support import env
    from vorbispizza_amd import Decoder, capi, make_packets
    c = b.case
    C_ = c["channels"]
    pk = make_packets(b.n)
    pk["flags"], pk["mapping"], pk["granule"], pk["residue_offset"] = b.flags, b.mapping, -1, b.residue_offset
    capfd.readouterr()
    with env(VPZ_NO_F0_FUSED=None if fused else 1, VPZ_HOST_PROFILE=1):
        dec = Decoder(ctx, C_, c["size0"], c["size1"], floors=b.floors, mappings=b.mappings)
        parts = []
        for a, e in zip(b.bounds[:-1], b.bounds[1:]):
            dec.set_floor0_data(b.amps[C_ * a:C_ * e], b.coeffs[C_ * a:C_ * e])
            parts.append(dec.synth(pk[a:e].copy(), b.res, b.posts[C_ * a:C_ * e], b.counts[C_ * a:C_ * e],
                                   out_layout=capi.OUT_PLANAR)[0])
        dec.close()
    routes = re.findall(r"\[vpz host\] packets \d+: route (\w+)", capfd.readouterr().err)
    return np.concatenate(parts, axis=1), routes


@pytest.mark.parametrize("case_id", fc.IDS)
def test_floor0_limits_match_the_oracle(ctx, oracle, capfd, case_id):
    b, ref = fc.built(case_id)
    assert np.isfinite(ref).all()
    bar = fc.TOL * max(1.0, float(np.abs(ref).max()))
    outs = {}
    for name in ("fused", "separate") if fc.fast_path(b.case) else ("separate",):
        got, routes = decode(ctx, b, name == "fused", capfd)
        outs[name] = got
        # (the route that ran is the one the case is about: the fast path applies the floor itself, the others after floor0_apply_kernel)
        assert routes == [fc.route(b.case, name == "fused")] * len(b.case["calls"]), routes
    for name, got in outs.items():  # (after the runs: capfd takes what is printed before a run with the run's own lines)
        assert got.shape == ref.shape
        err = float(np.abs(got.astype(np.float64) - ref).max())
        print("%s %s: |got - ref|max / max(1, |ref|max) = %.3g (the bar: %g)" % (case_id, name, err / (bar / fc.TOL), fc.TOL))
        assert np.isfinite(got).all() and err <= bar, (name, err, bar)
    if "fused" in outs:
        assert np.array_equal(outs["fused"].view(np.uint32), outs["separate"].view(np.uint32))
