"""Runners of the conv1 lattice checks on the GPU (raw bindings), shared by tests/test_gpu_exact_alexnet.py and by the
child processes it starts for the environment-selected kernel variants (the NIDT_C1* switches are read once per
process).  As a program: ``python _alexlattice_child.py case.pt`` runs the NB = 4 forward check and the NB = 4 slab check
on the operands and references the parent saved, with whatever variant the environment selects; it prints the
coordinates of the first mismatch and exits non-zero."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import _alexlattice as A  # noqa: E402

DEV = "cuda"
NAN = float("nan")
SENT = -96.0


def ext():
    from neuroimagedisttraining_amd import ops
    return ops.ext()


def _st():
    return torch.cuda.current_stream().cuda_stream


def run_pack(m, theta, P, off_w, off_sign, G, scale_arg):
    """pack_conv1_w into NaN / -1 initialised buffers sized from conv1_kslots()."""
    ks = m.conv1_kslots()
    w8 = torch.full((G, 64, ks), -1, dtype=torch.int16, device=DEV)
    w125 = torch.full((G, 64, 125), NAN, device=DEV)
    m.pack_conv1_w(theta.data_ptr(), P, off_w, off_sign, G, scale_arg, w8.data_ptr(), w125.data_ptr(), _st())
    return w8, w125


def run_fwd(m, x8, idx, w8, scale, shift, NB, B):
    """conv1_fwd_pool into NaN / 255 buffers with one guard sample behind the last."""
    out = torch.full((NB + 1, 19, 23, 19, 64), NAN, device=DEV).bfloat16()
    amax = torch.full((NB + 1, 19, 23, 19, 64), 255, dtype=torch.uint8, device=DEV)
    out[NB] = SENT
    m.conv1_fwd_pool(x8.data_ptr(), idx.data_ptr(), w8.data_ptr(), scale.data_ptr(), shift.data_ptr(), NB, B,
                     out.data_ptr(), amax.data_ptr(), _st())
    torch.cuda.synchronize()
    assert bool((out[NB].float() == SENT).all()) and bool((amax[NB] == 255).all()), "the guard sample was written"
    return out[:NB], amax[:NB]


def nslab(m, NB, B, mode):
    nq = m.conv1_wgrad_nq(NB)
    if mode == 2:
        npb = m.conv1_wgrad_mx_npb(NB)
        return B * ((19 + npb - 1) // npb)
    return B * 19 * nq


def run_wgrad(m, x8, idx, dp, pout, amax, NB, B, f):
    """conv1_wgrad with the closed-form operands f (A.fin_case) into a NaN part buffer and FILL gradient rows."""
    G = NB // B
    part = torch.full((NB * 19 * m.conv1_wgrad_nq(NB), 64, 126), NAN, device=DEV)
    grad = torch.full((G, f.ldg), A.FILL, device=DEV)
    theta = torch.full((G, 80), A.FILL, device=DEV)
    theta[:, 8:72] = f.gamma.to(DEV)
    t = {k: getattr(f, k).contiguous().to(DEV) for k in ("w125", "mu", "covw", "invstd")}
    em = None if f.emean is None else f.emean.contiguous().to(DEV)
    m.conv1_wgrad(x8.data_ptr(), idx.data_ptr(), dp.data_ptr(), pout.data_ptr(), amax.data_ptr(), NB, B,
                  part.data_ptr(), t["w125"].data_ptr(), t["mu"].data_ptr(), t["covw"].data_ptr(),
                  t["invstd"].data_ptr(), theta.data_ptr(), 80, 8, grad.data_ptr(), f.ldg, f.goff_w, f.goff_bias,
                  f.goff_g, f.goff_b, f.wscale, 0 if em is None else em.data_ptr(), _st())
    torch.cuda.synchronize()
    return part, grad


def check_slabs(part, G, nsl, S, D, what):
    assert bool(torch.isfinite(part[:G * nsl]).all()), what + ": a part slab entry was not written"
    gs, gd = A.part_sum(part.cpu(), G, nsl)
    e = A.first_mismatch(gs, S, ("client", "channel", "tap"))
    assert e is None, what + " S: " + e
    e = A.first_mismatch(gd, D, ("client", "channel"))
    assert e is None, what + " D: " + e


def main(path):
    d = torch.load(path)
    m = ext()
    c = d["c"]
    x8, idx = d["x8"].to(DEV), c["idx"].to(DEV)
    w8, _ = run_pack(m, c["theta"].to(DEV), c["P"], c["off_w"], c["off_sign"], c["G"], 1.0 / 255.0)
    out, amax = run_fwd(m, x8, idx, w8, c["scale"].to(DEV), c["shift"].to(DEV), c["NB"], c["B"])
    ref = type("C", (), {"out": c["out"], "amax": c["amax"]})
    A.check_conv1_fwd(out, amax, ref)
    print("forward ok (kslots %d)" % m.conv1_kslots())
    w = d["w"]
    mode = 2 if os.environ.get("NIDT_C1WG_MX", "1") == "1" else 0
    f = A.fin_case(c["G"], False)
    part, _ = run_wgrad(m, x8, idx, w["dp"].to(DEV), w["pout"].to(DEV), w["amax"].to(DEV), c["NB"], c["B"], f)
    check_slabs(part, c["G"], nslab(m, c["NB"], c["B"], mode), w["S"], w["D"], "slab sums (mode %d)" % mode)
    print("slab sums ok (mode %d)" % mode)


if __name__ == "__main__":
    try:
        main(sys.argv[1])
    except AssertionError as e:
        print("MISMATCH:", e)
        sys.exit(1)
