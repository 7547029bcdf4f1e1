"""The differential fuzzer of the fused lm_head + cross-entropy kernel (tests/test_score_gpu.py) at 8 x the case count: a long soak kept OUT of
`-m gpu` (run by hand with `pytest -m gpu_slow` on a GPU box, like tests/test_slow_gpu.py)."""
import pytest

pytestmark = pytest.mark.gpu_slow


def test_fused_head_differential_fuzz_long():
    from tests.test_score_gpu import _fuzz
    _fuzz(320, 8)
