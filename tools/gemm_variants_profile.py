#!/usr/bin/env python
"""Largest error of every instance of the generic GEMM kernel over the cases of tests/gemm_cases.py, in the unit of
tests/test_gpu_gemm_variants.py (|got - ref| / (|alpha| |a| @ |b| + |bias| + |c0|) against fp64): one line per operand-kind pair and
instance, with the case that produced it.  Needs the GPU.

    python tools/gemm_variants_profile.py [profiles/gemm_variants.txt]
"""
import contextlib
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "vibertgrid-pytorch_amd")):
    sys.path.insert(0, p)


def main():
    import gemm_cases as G
    import test_gpu_gemm_variants as T
    from vbg import ops
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gemm_variants.txt")
    worst, count, failed = {}, {}, []
    for c in G.CASES:
        key = (c.pair, c.expect[:5])
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                e = T.run_case(c, ops)
        except AssertionError as err:
            failed.append((c.name, str(err)[:200]))
            continue
        count[key] = count.get(key, 0) + 1
        if key not in worst or e > worst[key][0]:
            worst[key] = (e, c.name, G.bound_for(c.dims[2]))
    lines = ["# tools/gemm_variants_profile.py on an MI355X: largest error of each gemm_kernel instance over the cases of tests/gemm_cases.py,",
             "# |got - ref| / (|alpha| |a| @ |b| + |bias| + |c0|) against fp64 (bound: 2e-6 up to K = 640, 2e-6 sqrt(K / 640) beyond)",
             "# pair  BMxBNxBK  vec prec  cases  max_error  bound_of_that_case  case"]
    for pair in G.PAIRS:
        for v in G.INSTANCES[pair]:
            if (pair, v) in G.UNREACHABLE:
                lines.append(f"{pair}  {v[0]}x{v[1]}x{v[2]}  {v[3]} {v[4]}  unreachable")
                continue
            e, name, b = worst.get((pair, v), (float("nan"), "-", float("nan")))
            lines.append(f"{pair}  {v[0]}x{v[1]}x{v[2]}  {v[3]} {v[4]}  {count.get((pair, v), 0)}  {e:.3e}  {b:.3e}  {name}")
    for name, msg in failed:
        lines.append(f"# FAILED {name}: {msg}")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
