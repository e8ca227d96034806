"""The float64 restatement of the student step (tests/student_ref.py) against `Student.forward` run in float64 on the CPU and
against the reference's own step vectors in tests/golden/distill.npz.  CPU only."""
import os

import numpy as np
import torch

from locotouch_amd.distill import Student, distillation_cfg
from tests import distill_synth as S
from tests import student_ref as R

TASK = "Isaac-RandCylinderTransportStudent_SingleBinaryTac_CNNRNN_Mon-LocoTouch-v1"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distill.npz")


def make_student(tmp, seed):
    cfg = distillation_cfg(TASK)
    cfg.device, cfg.log_dir = "cpu", str(tmp)
    torch.manual_seed(seed)
    return Student(cfg, S.PROPRIO, S.TACTILE, S.ACTIONS, teacher_policy_inference=S.teacher_policy(), verbose=False).eval()


def test_restatement_equals_student_forward_in_float64_over_a_sequence_with_resets(tmp_path):
    st = make_student(tmp_path, 11).double()
    P = R.params_of(st)
    n, g = 7, torch.Generator().manual_seed(3)
    h, done = np.zeros((n, 512)), None
    st.reset()
    resets = 0
    with torch.no_grad():
        for t in range(20):
            prop = torch.randn(n, S.PROPRIO, generator=g, dtype=torch.float64)
            tac = torch.rand(n, S.TACTILE, generator=g, dtype=torch.float64) if t % 2 else (torch.rand(n, S.TACTILE, generator=g) < 0.1).double()
            want = st(prop, tac).numpy()
            got, h = R.step(P, prop.numpy(), tac.numpy(), h, done)
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
            np.testing.assert_allclose(h, st.get_hidden_states()[0].numpy(), rtol=0, atol=1e-12)
            dones = torch.rand(n, generator=g) < (1.0 if t == 5 else 0.0 if t == 6 else 0.3)
            resets += int(dones.sum())
            st.reset(dones)
            done = dones.numpy()
    assert resets > n


def test_restatement_equals_the_reference_step_vectors(tmp_path):
    gold = np.load(GOLD)
    st = make_student(tmp_path, 1234)  # the seed and inputs the fixture was recorded with (tests/test_distill.py)
    P = R.params_of(st)
    steps, _ = S.student_inputs()
    h = np.zeros((steps[0]["prop"].shape[0], 512))
    for i, s_ in enumerate(steps):
        y, h = R.step(P, s_["prop"].numpy(), s_["tac"].numpy(), h)
        np.testing.assert_allclose(y, gold["st_step_actions"][i], rtol=1e-5, atol=2e-6)
        assert abs(np.abs(h).sum() - gold["st_step_hidden_abs_sum"][i]) < 1e-3
        if i == 1:
            h = np.zeros_like(h)
