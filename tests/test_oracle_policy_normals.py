"""lt_oracle_policy_normals: the policy head's 12 N(0,1) draws per env in double - the Box-Muller transform of the Philox uniforms the
kernels key by (seed, env, step, stream 0x400 + action group), (u0, u1) -> actions 4q, 4q + 1 and (u2, u3) -> 4q + 2, 4q + 3.  The
uniforms come from an independent numpy Philox (tests/mlp_ref.rng4)."""
import numpy as np

from tests import mlp_ref as R
from tests import oracle_lib as O


def test_policy_normals_are_box_muller_of_the_keyed_uniforms():
    for seed, n, step in ((0x5EED_1234_ABCD, 300, 7), (3, 17, 0), (2**63 + 5, 40, 2**33 + 11)):
        z = O.policy_normals(seed, n, step)
        u = R.policy_uniforms(seed, n, step).astype(np.float64)  # [n][3][4]
        want = np.zeros((n, 12))
        for q in range(3):
            for h in range(2):
                r = np.sqrt(-2.0 * np.log(1.0 - u[:, q, 2 * h]))
                t = 2.0 * np.pi * u[:, q, 2 * h + 1]
                want[:, 4 * q + 2 * h], want[:, 4 * q + 2 * h + 1] = r * np.cos(t), r * np.sin(t)
        np.testing.assert_allclose(z, want, rtol=1e-13, atol=1e-13)
        assert z.dtype == np.float64 and np.isfinite(z).all()
    big = O.policy_normals(11, 20000, 3)
    assert abs(big.mean()) < 0.01 and abs(big.std() - 1.0) < 0.01  # N(0, 1)
    assert not np.array_equal(O.policy_normals(11, 8, 3), O.policy_normals(11, 8, 4))  # keyed by step
    # the f32 Box-Muller baseline of the GPU test is the same transform in float32
    np.testing.assert_allclose(R.policy_normals32(11, 64, 3).numpy(), O.policy_normals(11, 64, 3), rtol=0, atol=2e-5)
