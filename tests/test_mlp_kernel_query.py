"""lt_mlp_kernel_name (include/lt_env.h): the instantiation an MLP entry point launches, decided by the same host function as the launch
(launch_form in csrc/lt_mlp.hip).  Host-only.  The case table that covers every compiled instantiation is
tests/test_hip_mlp_f64.py::CASES (test_cases_cover_every_compiled_instantiation)."""
import ctypes

from locotouch_amd import _abi
from tests.test_hip_mlp_f64 import A270, A348, A348_BF16, C348, C_TANH, F1008, desc_of, kernel_name, row_tiles

C = _abi.CONSTS


def test_row_tiles_follow_the_batch_and_fall_back_where_lds_is_short():
    for mode, s1, one_net in (("fwd", None, True), ("pair", C348, False), ("policy", C348, False), ("policy", None, True), ("bwd", C348, False)):
        tiles = [row_tiles(mode, A348, s1, m) for m in (1, 4096, 8192, 16384, 32768, 1 << 20)]
        assert tiles == sorted(tiles) and tiles[0] == 1 and tiles[-1] == 4, (mode, tiles)
        # 16-row blocks of all networks: 2 from 512, 4 from 1024 (pick_row_tiles)
        blocks = 1 if one_net else 2
        assert row_tiles(mode, A348, s1, 16 * 512 // blocks) == 2 and row_tiles(mode, A348, s1, 16 * (512 // blocks - 1)) == 1, mode
        assert row_tiles(mode, A348, s1, 16 * 1024 // blocks) == 4 and row_tiles(mode, A348, s1, 16 * (1024 // blocks - 1)) == 2, mode
    # a 1008-wide input: 64 rows of 1012 floats do not fit 160 KiB of LDS - two row tiles where the batch asks for four
    assert kernel_name("fwd", F1008, None, 1 << 20) == "lt_mlp_kernel<2,1,1>"
    assert kernel_name("fwd", A348, None, 1 << 20) == "lt_mlp_kernel<4,1,1>"


def test_input_forms_of_a_pair():
    assert kernel_name("pair", A348, C348, 64) == "lt_mlp_kernel<1,1,1>"
    assert kernel_name("pair", A270, A270[:2] + (1,) + A270[3:], 64) == "lt_mlp_kernel<1,1,3>"
    assert kernel_name("pair", A348, A270, 64) == "lt_mlp_kernel<1,1,0>"  # different forms: run-time staging for both
    assert kernel_name("pair", A348_BF16, A348, 64) == "lt_mlp_kernel<1,1,0>"
    assert kernel_name("pair", A348, C_TANH, 64) == "lt_mlp_kernel<1,-1,0>"  # an ELU actor beside a tanh critic: generic activation
    assert kernel_name("bwd", A348, C348, 64) == "lt_mlp_kernel<1,100,0>"


def test_refused_shapes_name_no_kernel():
    lib = _abi.load()
    assert kernel_name("policy", A348[:2] + (13,) + A348[3:], None, 64) is None  # the policy head has 12 outputs
    assert kernel_name("pair", (348, (510, 256), 12, "elu", False), C348, 64) is None  # hidden widths % 4 (activations written by 4)
    assert kernel_name("fwd", (348, (510, 256), 12, "elu", False), None, 64) == "lt_mlp_kernel<1,1,1>"  # ... lt_mlp_forward takes them
    assert kernel_name("bwd", A348, C_TANH, 64) is None  # the backward chain gates by ELU'
    assert kernel_name("bwd", A348, None, 64) is None
    assert kernel_name("fwd", (348, (600,), 12, "elu", False), None, 64) is None  # outputs <= 512
    assert kernel_name("fwd", A348, None, 0) is None
    d = desc_of(A348)
    assert lib.lt_mlp_kernel_name(ctypes.byref(d), None, 64, 3) is None
    assert lib.lt_mlp_kernel_name(None, None, 64, C["LT_MLP_MODE_FORWARD"]) is None
