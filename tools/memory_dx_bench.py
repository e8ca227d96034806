"""The input gradient of the two memories, dx = d_ih W_ih for both networks: `lt_memory_input_grad` (include/lt_memory_dx.h, ONE launch)
against the library product, `torch.mm(d_ih, w_ih, out=dx)` once per network.  Shapes: n rows (24 576 = a rollout of 24 steps x 1024
envs), I = 64 for both networks, K = 768 (a GRU of H = 256) and K = 1024 (an LSTM of H = 256).

One fresh process per leg and shape; after `--warmup` calls, `--rounds` (7) rounds of `--iters` back-to-back calls between two events on
the stream; per call: the median of the rounds with [min, max].  `gb_per_s_of_dg` is the bytes of the two dg arrays - what the call must
read at least, 75 to 100 MB per network at these shapes - over the median: a whole-call rate, not a kernel's share of peak, and with
back-to-back calls on the same arrays not an HBM rate either (the 256 MiB last-level cache can hold them).  The kernel
keeps ONE fixed summation order and writes rows of any stride in place; the library product promises neither, so the comparison records
what that costs or saves - it selects nothing.  Results: profiles/memory_dx_<n>.json."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SHAPES = {"gru": (3, 256), "lstm": (4, 256)}  # name: (gates, H)
LEGS = ("hip", "mm")


def stats(v: list) -> dict:
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1]}


def tree():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:  # noqa: BLE001
        return None


def measure(leg: str, shape: str, n: int, I: int, rounds: int, warmup: int, iters: int) -> dict:
    import torch

    from locotouch_amd import _abi

    if not torch.cuda.is_available():
        sys.exit("memory_dx_bench: no GPU: a time is measured on the device or not at all")
    gates, H = SHAPES[shape]
    K = gates * H
    g = torch.Generator(device="cuda").manual_seed(1)
    dgs = [torch.randn(n, K, device="cuda", generator=g) for _ in range(2)]
    ws = [torch.randn(K, I, device="cuda", generator=g) * I ** -0.5 for _ in range(2)]
    dxs = [torch.empty(n, I, device="cuda") for _ in range(2)]
    if leg == "hip":
        nets = [_abi.LtMemoryDxNet(dg=d.data_ptr(), w_ih=w.data_ptr(), I=I, dx=x.data_ptr(), dx_stride=I) for d, w, x in zip(dgs, ws, dxs)]
        stream = _abi.stream(torch.device("cuda:0"))

        def call():
            _abi.call("lt_memory_input_grad", nets[0], nets[1], n, H, gates, stream)
    else:
        def call():
            for d, w, x in zip(dgs, ws, dxs):
                torch.mm(d, w, out=x)
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    ref = [d.double() @ w.double() for d, w in zip(dgs, ws)]
    err = max(float((x.double() - r).abs().max()) for x, r in zip(dxs, ref))
    out = {"leg": leg, "shape": shape, "gates": gates, "H": H, "K": K, "I": I, "n": n, "iters": iters, "ms_per_call": stats(ms),
           "dg_bytes": 2 * n * K * 4, "max_abs_err_vs_f64": err}
    out["gb_per_s_of_dg"] = out["dg_bytes"] / (out["ms_per_call"]["median"] * 1e-3) / 1e9
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=24576)
    ap.add_argument("--I", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", help="what to record as measured_on_commit (default: git rev-parse --short HEAD, null outside a checkout)")
    ap.add_argument("--leg", choices=LEGS, help="measure one leg of one --shape in this process and print its RESULT line")
    ap.add_argument("--shape", choices=list(SHAPES))
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("--rounds must be at least 5")
    if args.leg:
        print("RESULT " + json.dumps(measure(args.leg, args.shape or "gru", args.n, args.I, args.rounds, args.warmup, args.iters)))
        return
    cases = {}
    for shape in SHAPES:
        legs = {}
        for leg in LEGS:  # a fresh process each: no allocator or library state carried from one to the next
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--shape", shape, "--n", str(args.n), "--I", str(args.I),
                                "--rounds", str(args.rounds), "--warmup", str(args.warmup), "--iters", str(args.iters)],
                               capture_output=True, text=True, timeout=300)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit(f"{shape} {leg}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            legs[leg] = json.loads(line[-1][7:])
            print(line[-1], flush=True)
        h, m = legs["hip"]["ms_per_call"], legs["mm"]["ms_per_call"]
        cases[shape] = {"legs": legs, "mm_over_hip_ratio_of_medians": m["median"] / h["median"],
                        "intervals_overlap": h["min"] <= m["max"] and m["min"] <= h["max"]}
    res = {"n": args.n, "I": args.I, "measured_on_commit": args.commit or tree(),
           "notes": {"ms_per_call": "events on the stream around `iters` back-to-back calls, both networks per call; median [min, max] over the rounds",
                     "hip": "lt_memory_input_grad, one launch for both networks", "mm": "torch.mm(d_ih, w_ih, out=dx), one call per network",
                     "gb_per_s_of_dg": "bytes of the two dg arrays over the median time of a call: a whole-call rate, not a share of peak - and "
                                       "no HBM rate either: back-to-back calls re-read the same 150 to 200 MB, which the 256 MiB last-level cache can hold",
                     "claim": "none: the HIP form is kept for its fixed summation order and its in-place strided output whichever way this falls"},
           "cases": cases}
    out = args.out or os.path.join(REPO, "profiles", f"memory_dx_{args.n}.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"hip": v["legs"]["hip"]["ms_per_call"], "mm": v["legs"]["mm"]["ms_per_call"]} for k, v in cases.items()}))


if __name__ == "__main__":
    main()
