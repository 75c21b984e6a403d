"""Which explicit form reproduces torch's lerp bits on this device?  Runs the four candidates of tools/probes/lerp_form_probe.hip
(build line in that file: contraction must be off) against torch._foreach_lerp_, torch.lerp with a Python weight and torch.lerp with
a tensor weight, on 2^20 elements spread over many binades (a quarter of them with p within 1e-3 of a), and prints per weight the
number of elements whose bits differ.  form 0: every operation rounded on its own; 1: first branch fused; 2: second branch fused;
3: both.  The result decided vbg_lerp's statement (csrc/optim.hip, profiles/weight_average.txt).  Needs the GPU.

    python tools/lerp_form_probe.py [path/to/liblerp_form_probe.so]"""
import ctypes as C
import os
import sys

import torch

WEIGHTS = (1 - 0.999, 1 - 0.9999, 1 / 3, 0.49999, 0.5, 0.75, 1.0, 0.0, 0.9, -0.25, 1.5)


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "probes", "liblerp_form_probe.so")
    lib = C.CDLL(path)
    lib.probe_lerp.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_float, C.c_int, C.c_void_p]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    n = 1 << 20
    a = (torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * 3)).to(dev)
    p = (torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * 3)).to(dev)
    p[: n // 4] = a[: n // 4] * (1 + 1e-3 * torch.randn(n // 4, device=dev))
    for w in WEIGHTS:
        ref = a.clone()
        torch._foreach_lerp_([ref], [p], w)
        line = [f"w={w:<22}", f"foreach==lerp {torch.equal(ref, torch.lerp(a, p, w))}",
                f"tensor-w==lerp {torch.equal(ref, torch.lerp(a, p, torch.tensor(w, device=dev)))}"]
        for form in range(4):
            out = a.clone()
            rc = lib.probe_lerp(out.data_ptr(), p.data_ptr(), n, w, form, None)
            torch.cuda.synchronize()
            assert rc == 0, rc
            line.append(f"form{form}: {int((out.view(torch.int32) != ref.view(torch.int32)).sum())}")
        print("  ".join(line), flush=True)
    print(torch.__version__, torch.cuda.get_device_name(0))


if __name__ == "__main__":
    main()
