"""CPU half of tests/test_gpu_ekf_dispatch.py: the host mirror of the down-date dispatch, the coverage of its GPU grids,
and the observe() inputs those grids build (checked with the oracle on an fp32-rounded state, as the device holds it)."""
import numpy as np
import pytest

from tests.test_gpu_ekf_dispatch import (FALLBACKS, LABELS, OBSERVE_CELLS, _observe_oracle, expected_path, grid_paths, observe_inputs,
                                         observe_state)


def test_the_gpu_grids_reach_every_downdate_body():
    """If the dispatch gains or loses a body, expected_path and this list change with it."""
    paths = grid_paths()
    assert {label for label, _ in paths} == set(LABELS)
    # observe(): the device's count keeps the host's body, falls back to dd_tile inside the launch, or skips the down-date
    assert {fb for _, fb in paths} == set(FALLBACKS)


@pytest.mark.parametrize("dtype,form,m,xflags,device_m,want", [
    ("f32", "cholesky", 16, 0, None, ("f32_tile", None)),               # kp_total 32: no streaming path
    ("f32", "cholesky", 17, 0, None, ("f32_stream2", None)),            # kp_total 48: a half second chunk
    ("f32", "cholesky", 33, 0, None, ("f32_bf16_claim", None)),         # kp_total 80
    ("f32", "cholesky", 33, 8, None, ("f32_stream3", None)),
    ("f32", "cholesky", 64, 8, None, ("f32_stream4", None)),
    ("f32", "cholesky", 64, 16, None, ("f32_bf16_list", None)),
    ("f32", "cholesky", 64, 4, None, ("f32_tile", None)),
    ("f32", "cholesky", 64, 1024, None, ("f32_bf16_claim", None)),      # an experiments-build bit: masked in the product
    ("f32", "cholesky", 65, 0, None, ("f32_global_factor+tile", None)),
    ("f32", "joseph", 16, 0, None, ("f32_stream2", None)),              # 2 * 32
    ("f32", "joseph", 17, 0, None, ("f32_stream4_joseph", None)),       # 2 * 64
    ("f32", "joseph", 33, 0, None, ("f32_tile", None)),                 # 2 * 96
    ("f32", "joseph", 65, 0, None, ("f32_global_factor+tile", None)),
    ("f32", "cholesky", 64, 0, 40, ("f32_bf16_claim", None)),           # device kp 80
    ("f32", "cholesky", 64, 0, 20, ("f32_bf16_claim", "dd_tile")),      # device kp 48
    ("f32", "cholesky", 64, 0, 0, ("f32_bf16_claim", "skip")),
    ("f32", "cholesky", 64, 8, 50, ("f32_stream4", None)),              # device kp 112: still four chunks
    ("f32", "cholesky", 64, 8, 40, ("f32_stream4", "dd_tile")),         # device kp 80: three
    ("f32", "cholesky", 70, 0, 60, ("f32_global_factor+tile", None)),
    ("f64", "joseph", 33, 0, 0, ("f64", "skip")),
])
def test_expected_path_cases(dtype, form, m, xflags, device_m, want):
    assert expected_path(dtype, form, m, xflags, device_m) == want


@pytest.mark.parametrize("N,nz,j", OBSERVE_CELLS)
def test_observe_inputs_give_the_intended_counts(N, nz, j):
    """The GPU test's observations, built from the same seed on the same fp32-rounded state: the oracle matches exactly j of
    them and drops the others (between the gates), so the device count is j while the host's bound is nz."""
    rng = np.random.default_rng(40_000 * N + 100 * nz + j)
    x, P = observe_state(rng, N)
    xo = x.astype(np.float32).astype(np.float64)
    Po = P.astype(np.float32).astype(np.float64)
    _observe_oracle(xo, Po, observe_inputs(rng, xo, Po, N, nz, j), j, 0)
