#!/usr/bin/env python3
"""Cost of deterministic mode at the bench workload (cfg2, batch 8, one MI355X): bench.py's step timed with VBG_DETERMINISTIC=0 and =1,
in fp32 and with --amp, alternating the two settings over `--reps` fresh processes (each with its own warm-up; the JSON line's median),
and the medians of those reported.  Writes profiles/determinism_cost.txt (or --out).

    python tools/determinism_cost.py --steps 20 --warmup 5 --reps 3
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(det, amp, steps, warmup, timeout):
    env = dict(os.environ, VBG_DETERMINISTIC="1" if det else "0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    if amp:
        cmd.append("--amp")
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if out.returncode != 0:
        raise SystemExit(f"bench.py exited with {out.returncode} (det={det}, amp={amp}):\n{out.stderr[-3000:]}")
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "determinism_cost.txt"))
    a = ap.parse_args()
    rows = []
    for amp in (False, True):
        vals = {False: [], True: []}
        for _ in range(a.reps):
            for det in (False, True):           # alternate: drift of the machine lands on both settings alike
                r = one(det, amp, a.steps, a.warmup, a.timeout)
                vals[det].append(float(r["value"]))
        off, on = statistics.median(vals[False]), statistics.median(vals[True])
        rows.append((("amp" if amp else "fp32"), off, on, vals))
    lines = ["deterministic mode cost, bench.py cfg2 batch 8 (value = bench.py headline, higher is better); "
             f"{a.reps} processes per setting, {a.steps} steps after {a.warmup} warm-up each, medians"]
    for form, off, on, vals in rows:
        lines.append(f"{form}: off {off:.4g}  on {on:.4g}  on/off {on / off:.4f}  (overhead {100 * (off / on - 1):.1f} % step time)"
                     f"  runs off {vals[False]} on {vals[True]}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
