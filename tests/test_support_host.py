"""tests/support.py and tools/bench_support.py without a GPU: the comparison rules pass exactly at their bound and fail one fp64 ulp above
it, the seeded draws are those of the helpers they replaced, the bit and ulp helpers, and both modules import without a device or library."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _above(v):
    return math.nextafter(v, math.inf)


@pytest.mark.parametrize('tol, scale', [(1e-4, 3.0), (0.25, 2.0), (1e-4, 1e-9)])
def test_close_at_and_above_the_bound(tol, scale):
    """b = (scale, 0): the second element's error is a itself, so the error equals any fp64 limit exactly.  scale 1e-9: the 1e-6 floor."""
    lim = tol * max(scale, 1e-6)
    b = torch.tensor([scale, 0.0], dtype=torch.float64)
    support.close(torch.tensor([scale, lim], dtype=torch.float64), b, tol, 'at')
    support.close(torch.tensor([scale, -lim], dtype=torch.float64), b.numpy(), tol, 'at, numpy reference')
    with pytest.raises(AssertionError, match='above'):
        support.close(torch.tensor([scale, _above(lim)], dtype=torch.float64), b, tol, 'above')


def test_close_atol_replaces_the_relative_limit():
    b = torch.tensor([1000.0, 0.0], dtype=torch.float64)
    atol = 2e-3
    support.close(torch.tensor([1000.0, atol], dtype=torch.float64), b, None, 'at', atol=atol)
    support.close(torch.tensor([1000.0, atol], dtype=torch.float64), b, 1e-12, 'tol is not consulted', atol=atol)
    with pytest.raises(AssertionError, match='above'):
        support.close(torch.tensor([1000.0, _above(atol)], dtype=torch.float64), b, None, 'above', atol=atol)
    with pytest.raises(AssertionError, match='relative'):      # 2e-3 is inside tol * scale = 0.1, and outside atol = 1e-3
        support.close(torch.tensor([1000.0, atol], dtype=torch.float64), b, 1e-4, 'relative', atol=1e-3)


def test_close_and_close_elem_refuse_a_shape_mismatch():
    with pytest.raises(AssertionError):
        support.close(torch.zeros(2, 3), torch.zeros(3, 2), 1.0, 'shape')
    with pytest.raises(AssertionError):
        support.close_elem(torch.zeros(6), torch.zeros(2, 3), 'shape')


def test_close_elem_at_and_above_the_bound_counts_the_offenders():
    """b = (2, 0, 0, 0): rms(b) = 1 exactly, so a zero element's limit is atol and the first element's rtol * 2 + atol."""
    rtol, atol = 2.0 ** -13, 2.0 ** -17                         # powers of two: every limit below is exact in fp64
    b = torch.tensor([2.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    at = torch.tensor([2.0 + (2.0 * rtol + atol), atol, -atol, 0.0], dtype=torch.float64)
    support.close_elem(at, b, 'at', rtol=rtol, atol=atol)
    above = at.clone()
    above[1], above[2] = _above(atol), -_above(atol)
    with pytest.raises(AssertionError, match='2 of 4 elements outside'):
        support.close_elem(above, b, 'above', rtol=rtol, atol=atol)
    above[0] = _above(float(at[0]))
    with pytest.raises(AssertionError, match='3 of 4 elements outside'):
        support.close_elem(above, b.numpy(), 'above', rtol=rtol, atol=atol)
    support.close_elem(b.float(), b, 'defaults')


def test_rnd_draws_what_the_replaced_helpers_drew():
    """The expressions are test_gpu_ops.py::rnd and test_dcn2d_host.py::rnd as they stood before tests/support.py."""
    seed, shape = 3, (2, 5)
    f32 = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    assert torch.equal(support.rnd(*shape, seed=seed), f32 * 1.0) and support.rnd(*shape, seed=seed).dtype == torch.float32
    assert torch.equal(support.rnd(*shape, seed=seed), f32)                                      # the variant without a scale
    assert torch.equal(support.rnd(*shape, seed=seed, scale=0.5), f32 * 0.5)
    f64 = torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    assert torch.equal(support.rnd(*shape, seed=seed, dtype=torch.float64), f64 * 1.0)
    assert torch.equal(support.rnd(*shape, seed=seed, scale=0.5, dtype=torch.float64), f64 * 0.5)


def test_ulp_helpers():
    assert support.ulp_of(1.0) == 2.0 ** -23 and support.ulp_of(-1.0) == 2.0 ** -23 and support.ulp_of(3.0) == 2.0 ** -22
    assert support.ulp_of_max(np.zeros((0, 3))) == 0.0
    assert support.ulp_of_max(np.array([0.5, -3.0, 1.0])) == 2.0 ** -22


def test_bits_round_trips_a_nan_payload_and_negative_zero():
    patterns = np.array([0x7FC12345, 0xFFC00001, 0x80000000, 0x00000000, 0x3F800000], dtype=np.uint32)
    values = patterns.view(np.float32)
    assert np.array_equal(support.bits(values), patterns)
    assert np.array_equal(support.bits(values).view(np.float32).view(np.uint32), patterns)
    assert not np.array_equal(support.bits(np.float32(-0.0)), support.bits(np.float32(0.0)))
    assert support.bits(values[::2]).flags['C_CONTIGUOUS']


@pytest.mark.parametrize('statement, path', [('import tests.support', ROOT), ('import bench_support', os.path.join(ROOT, 'tools'))])
def test_support_modules_import_without_a_device_or_the_library(statement, path, tmp_path):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES='', DPF_LIB_PATH=str(tmp_path / 'missing' / 'libdpf_hip.so'), PYTHONPATH=path)
    check = statement + "; import sys; assert not [m for m in sys.modules if m.startswith('dualpixelface_amd')]"
    done = subprocess.run([sys.executable, '-c', check], env=env, cwd=str(tmp_path), capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
