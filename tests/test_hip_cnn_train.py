"""The training form of the tactile CNN head (csrc/lt_cnn_train.hip behind include/lt_cnn_train.h, locotouch_amd/rl/cnn_train.py) on the
GPU.  The reference is `CNN2dHead` in float64 on the CPU (plain nn.Conv2d semantics, torch autograd).  The eager f32 GPU module (the
parent's path) only sizes the tolerance: per gradient tensor the bound is 4 x the eager module's own error against the same f64 reference,
both normalised by the tensor's max |grad| (two f32 accumulations of the same length in different orders).

Near-ties are a discontinuity.  The near-tie set of the issue: an image is in it if, in f64, some max-pool window's top two values differ
by less than 1e-5 of the map's max, or some ReLU pre-activation is within that of 0.  Taken literally that set holds 8-17 % of seeded normal
images of the registered stack whatever the seed (3912 pre-activations and 840 windows per image), far above the 2 % the left-out share may
reach.  So the comparison leaves out only the SUBSET of it whose tie can reach a gradient at all - every other image of the set stays in,
which asks more of the kernels, not less:
  - behind a pool only a window's maximum passes gradient, so what counts there is the window's maximum within the margin of 0, or its top
    two pre-activations within the margin of each other with a positive maximum (a pre-activation that is not its window's maximum, or lies
    in a row / column the pool's floor drops, gets no gradient on either side of 0); a layer without a pool counts every pre-activation;
  - the margin is 1e-5 of max |z| of the map the value lies in (one image, one channel);
  - an image whose d_emb row is exactly zero (a padded step) adds exact zeros to every gradient whatever its ties: it stays in.
PARAM_SEED and SEEDS are picked, on the CPU, so that this left-out share of the f64 reference alone is <= 2 % for every case
(`test_left_out_share_of_the_f64_reference`; at N < 50 that means no image is left out)."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

gpu = pytest.mark.gpu
DEV = "cuda:0"
REG = dict(img=(2, 17, 13), channels=(24, 24, 24), kernels=(4, 3, 2), strides=(2, 1, 1), pool=True, out=64)
ONE = dict(img=(1, 9, 8), channels=(5,), kernels=(3,), strides=(1,), pool=False, out=16)          # one convolution, no pool
ODD = dict(img=(2, 11, 9), channels=(5, 7), kernels=(3, 2), strides=(2, 1), pool=True, out=16)  # conv 1 gives 9 x 7: the floor drops a row and a column
STR = dict(img=(2, 12, 11), channels=(5, 6), kernels=(3, 2), strides=(2, 2), pool=False, out=16)  # strided convolutions, no pool: 5 x 5, then 2 x 2
CASES = ([(REG, n) for n in (1, 7, 8, 9, 100, 2051)] + [(ONE, n) for n in (1, 9, 100)] + [(ODD, n) for n in (1, 9, 100)]
         + [(STR, n) for n in (9, 100)])
PARAM_SEED = 27
SEEDS = {("reg", 1): 1, ("reg", 7): 1, ("reg", 8): 2, ("reg", 9): 2, ("reg", 100): 2, ("reg", 2051): 2, ("one", 1): 1, ("one", 9): 1,
         ("one", 100): 1, ("odd", 1): 1, ("odd", 9): 1, ("odd", 100): 1, ("str", 9): 1, ("str", 100): 2}  # (stack, N) -> seed of the images and d_emb


def make_head(spec, dtype, device):
    import torch

    from locotouch_amd.rl.models import CNN2dHead

    torch.manual_seed(PARAM_SEED)
    head = CNN2dHead(spec["img"], spec["channels"], spec["kernels"], spec["strides"], None, None, spec["out"], "relu", spec["pool"])
    return head.to(dtype=dtype, device=device)


def grads_of(head, x, d_emb):
    """[gradient of sum(emb * d_emb) per parameter], emb"""
    import torch

    params = list(head.parameters())
    emb = head(x)
    return [g.detach() for g in torch.autograd.grad((emb * d_emb).sum(), params)], emb.detach()


def near_ties(head64, x64, d_emb):
    """bool [N]: the images left out of a gradient comparison (module docstring), from the f64 forward."""
    import torch
    import torch.nn.functional as F

    n = x64.shape[0]
    mods = list(head64.conv.conv)
    bad, a, z = torch.zeros(n, dtype=torch.bool), x64, None
    with torch.no_grad():
        for i, m in enumerate(mods):
            if isinstance(m, torch.nn.Conv2d):
                z = a = F.conv2d(a, m.weight, m.bias)
                tol = 1e-5 * z.abs().amax((2, 3), keepdim=True)
                if not (i + 2 < len(mods) and isinstance(mods[i + 2], torch.nn.MaxPool2d)):
                    bad |= (z.abs() < tol).flatten(1).any(1)
            elif isinstance(m, torch.nn.ReLU):
                a = F.relu(a)
            else:
                k = m.kernel_size
                top = F.unfold(z, k, stride=k).view(n, z.shape[1], k * k, -1).topk(2, dim=2).values
                t = tol.flatten(2)
                bad |= ((top[:, :, 0].abs() < t) | ((top[:, :, 0] - top[:, :, 1] < t) & (top[:, :, 0] > 0))).flatten(1).any(1)
                a = F.max_pool2d(a, k)
    return bad & (d_emb != 0).any(1)


def name_of(spec):
    return "reg" if spec is REG else "one" if spec is ONE else "odd" if spec is ODD else "str"


IDS = [f"{name_of(s)}-{n}" for s, n in CASES]


def real_inputs(spec, n, seed=None):
    """Seeded normal images, d_emb normal with about a quarter of the rows exactly zero (as padded steps are)."""
    import torch

    g = torch.Generator().manual_seed(SEEDS[name_of(spec), n] if seed is None else seed)
    c, h, w = spec["img"]
    x = torch.randn(n, c, h, w, generator=g)
    live = torch.rand(n, 1, generator=g) >= 0.25
    live[0] = True  # (N = 1 needs a gradient to compare)
    return x, torch.randn(n, spec["out"], generator=g) * live


def binary_inputs(spec, reps=4):
    """The task's real input: all-zero, all-one, stripes constant along x, stripes constant along y, Bernoulli(0.1); ties are exact."""
    import torch

    g = torch.Generator().manual_seed(3)
    c, h, w = spec["img"]
    ys, xs = torch.arange(h).view(1, h, 1).expand(c, h, w), torch.arange(w).view(1, 1, w).expand(c, h, w)
    kinds = [torch.zeros(c, h, w), torch.ones(c, h, w), (ys % 2 == 0).float(), (xs % 2 == 0).float(), ((ys // 2) % 2 == 0).float(),
             ((xs // 2) % 2 == 1).float()] + [(torch.rand(c, h, w, generator=g) < 0.1).float() for _ in range(reps)]
    x = torch.stack(kinds)
    return x, torch.randn(x.shape[0], spec["out"], generator=g)


def compare(spec, x, d_emb, keep=None):
    """Per parameter: (our normalised error, the eager f32 GPU module's) against f64 on the rows `keep`; our emb and the f64 one."""
    import torch

    if keep is not None:
        x, d_emb = x[keep], d_emb[keep]
    n = x.shape[0]
    head64 = make_head(spec, torch.float64, "cpu")
    ref, emb64 = grads_of(head64, x.double(), d_emb.double())
    fused = make_head(spec, torch.float32, DEV)
    fused.enable_fused_training(spec["img"])
    ours, emb = grads_of(fused, x.to(DEV), d_emb.to(DEV))
    # the eager module on its training path (`Conv2dAsGemm`'s GEMM form needs N >= 1024): zero images with zero d_emb rows add exact zeros
    eager = make_head(spec, torch.float32, DEV)
    pad = max(0, 1024 - n)
    xe = torch.cat([x, torch.zeros(pad, *x.shape[1:])]).to(DEV)
    de = torch.cat([d_emb, torch.zeros(pad, d_emb.shape[1])]).to(DEV)
    theirs, _ = grads_of(eager, xe, de)
    rows = []
    for (name, _), r, o, t in zip(head64.named_parameters(), ref, ours, theirs):
        scale = r.abs().max().item()
        rows.append((name, (o.double().cpu() - r).abs().max().item() / scale, (t.double().cpu() - r).abs().max().item() / scale))
    return rows, emb, emb64


def check(rows, what):
    worst = 0.0
    for name, ours, theirs in rows:
        print(f"{what}: {name}: ours {ours:.3e}  eager f32 {theirs:.3e}  ratio {ours / theirs if theirs else float('inf'):.2f}")
        worst = max(worst, ours / theirs if theirs else float("inf"))
    for name, ours, theirs in rows:
        assert ours <= 4.0 * theirs, (what, name, ours, theirs)
    return worst


@pytest.mark.parametrize("spec, n", CASES, ids=IDS)
def test_left_out_share_of_the_f64_reference(spec, n):
    """CPU only: the reference alone stays under the cap for the fixed seeds."""
    import torch

    x, d_emb = real_inputs(spec, n)
    share = near_ties(make_head(spec, torch.float64, "cpu"), x.double(), d_emb).float().mean().item()
    print(f"left-out share: {share:.4f}")
    assert share <= 0.02, share


@gpu
@pytest.mark.parametrize("spec, n", CASES, ids=IDS)
def test_forward_and_backward_on_real_valued_images(spec, n):
    import torch

    x, d_emb = real_inputs(spec, n)
    keep = ~near_ties(make_head(spec, torch.float64, "cpu"), x.double(), d_emb)
    print(f"left out as near-ties: {1 - keep.float().mean().item():.4f}")
    assert keep.float().mean().item() >= 0.98
    rows, emb, emb64 = compare(spec, x, d_emb, keep)
    scale = emb64.abs().max().item()
    err = (emb.double().cpu() - emb64).abs().max().item() / scale
    print(f"emb: normalised error {err:.3e}")
    assert err < 2e-6  # f32 dot products of <= 216 + 192 terms against f64: a few eps of the largest value
    check(rows, f"N = {n}")


@gpu
def test_rows_do_not_depend_on_n_or_place():
    import torch

    head = make_head(REG, torch.float32, DEV)
    head.enable_fused_training(REG["img"])
    x, _ = real_inputs(REG, 100)
    x = x.to(DEV)
    big = head(x)
    assert torch.equal(head(x[:9]), big[:9]) and torch.equal(head(x[50:59].flatten(1)), big[50:59])
    with torch.no_grad():
        assert torch.equal(head(x), make_head(REG, torch.float32, DEV)(x))   # no_grad keeps the module path, bit for bit


@gpu
@pytest.mark.parametrize("spec", [REG, ONE, ODD, STR], ids=["reg", "one", "odd", "str"])
def test_backward_on_binary_images(spec):
    x, d_emb = binary_inputs(spec)
    rows, emb, emb64 = compare(spec, x, d_emb)
    assert (emb.double().cpu() - emb64).abs().max().item() / emb64.abs().max().item() < 2e-6
    check(rows, "binary")


@gpu
def test_gradients_are_reproducible_and_overwritten():
    import torch

    from locotouch_amd import _abi
    from locotouch_amd.rl.cnn_train import _pointers, describe_cnn

    n = 2051
    head = make_head(REG, torch.float32, DEV)
    desc, params = describe_cnn(head, REG["img"])
    params = [p.detach() for p in params]
    x, d_emb = (t.to(DEV) for t in real_inputs(REG, n))
    x = x.flatten(1).contiguous()
    size = ctypes.c_size_t()
    _abi.call("lt_cnn_ws_floats", desc, n, ctypes.byref(size))
    runs = []
    for fill in (0.0, float("nan"), 7.0):
        grads = [torch.full_like(p, fill) for p in params]
        ws = torch.full((size.value,), fill, device=DEV)
        _abi.call("lt_cnn_backward", desc, _pointers(_abi.LtCnnParams(), 3, params), x, d_emb, n, _pointers(_abi.LtCnnGrads(), 3, grads), ws,
                  _abi.stream())
        runs.append(grads)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.isfinite(b).all() and torch.equal(a, b)


@gpu
def test_autograd_front_through_the_student(tmp_path):
    import torch

    from locotouch_amd.distill import Student, distillation_cfg
    from tests.distill_synth import student_inputs, teacher_policy

    teacher = teacher_policy()

    def student(device):
        cfg = distillation_cfg("Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1")
        cfg.device, cfg.log_dir = device, str(tmp_path)
        torch.manual_seed(5)
        return Student(cfg, 270, 442, 12, teacher_policy_inference=lambda obs: teacher(obs.float().cpu()).to(obs), verbose=False)

    _, batch = student_inputs(L=7, B=3)
    grads = []
    for fused in (False, True, None):   # None: the f64 reference on the CPU
        s = student("cpu" if fused is None else DEV)
        if fused:
            s.pre_encoder.enable_fused_training(s.tactile_signal_img_shape)
        if fused is None:
            s = s.double()
        b = {k: v.to(device=s.device, dtype=torch.float64 if fused is None and v.is_floating_point() else v.dtype) for k, v in batch.items()}
        if fused is False:
            # the eager module on its training path (`Conv2dAsGemm`'s GEMM form needs L * B >= 1024, as a real batch has): 144 more columns of
            # masked padding, which add exact zeros to the loss and to every gradient
            b = {k: torch.cat([v, v.new_zeros(v.shape[0], 144, *v.shape[2:])], dim=1) for k, v in b.items()}
        loss, _, _ = s.batch_loss(b)
        loss.backward()
        grads.append({k: p.grad.double().cpu() for k, p in s.pre_encoder.named_parameters()})
    eager, ours, ref = grads
    for k in ref:
        scale = ref[k].abs().max().item()
        e_ours, e_eager = (ours[k] - ref[k]).abs().max().item() / scale, (eager[k] - ref[k]).abs().max().item() / scale
        print(f"{k}: ours {e_ours:.3e}  eager {e_eager:.3e}")
        assert e_ours <= 4.0 * e_eager, (k, e_ours, e_eager)


@gpu
def test_the_front_refuses_an_input_that_needs_a_gradient():
    import torch

    head = make_head(REG, torch.float32, DEV)
    head.enable_fused_training(REG["img"])
    x = torch.randn(4, 2, 17, 13, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match="input"):
        head(x)
    with pytest.raises(ValueError, match="CUDA"):
        make_head(REG, torch.float32, "cpu").enable_fused_training(REG["img"])
    with pytest.raises(ValueError, match="float32"):
        make_head(REG, torch.float64, DEV).enable_fused_training(REG["img"])


@gpu
def test_launch_count(tmp_path):
    """lt_cnn_launches against a kernel trace of one forward and one backward in a fresh child process (the profiled program after `--`)."""
    import csv
    import glob

    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    assert os.path.exists(rocprof), "rocprofv3 is needed for the launch count"
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=repo + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "300", rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(tmp_path), "-o", "trace", "--",
           sys.executable, os.path.join(repo, "tests", "_cnn_train_child.py"), "2051"]
    out = subprocess.run(cmd, cwd=repo, env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    fwd, bwd = (int(v) for v in [ln for ln in out.stdout.splitlines() if ln.startswith("LAUNCHES")][0].split()[1:])
    files = glob.glob(os.path.join(str(tmp_path), "**", "*kernel_trace.csv"), recursive=True)
    assert files, [os.path.join(d, f) for d, _, fs in os.walk(tmp_path) for f in fs]
    rows = sorted((row for f in files for row in csv.DictReader(open(f)) if "lt_cnn" in row["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    kinds = [next(k for k in ("pack", "forward", "backward", "reduce") if f"lt_cnn_{k}_kernel" in r["Kernel_Name"]) for r in rows]
    print("kernels in launch order:", kinds)
    cut = kinds.index("forward") + 1   # the child calls lt_cnn_forward, then lt_cnn_backward
    assert kinds[:cut] == ["pack", "forward"] and len(kinds[:cut]) == fwd
    assert kinds[cut:] == ["pack", "backward", "reduce"] and len(kinds[cut:]) == bwd
