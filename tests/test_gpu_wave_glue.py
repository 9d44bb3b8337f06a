"""fused_add_rmsnorm with the row held in registers (rmsnorm_wide_reg_kernel)
against the kernel it replaces (rmsnorm_wide_kernel): torch.equal on the
normalized output and on the updated residual. qkv_prep has no new variant
(none cleared the routing margin, profiles/PROFILES.md capture A1), so it has
no test here."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sutro_amd import ops
    from sutro_amd.ops import torch_ref as R
else:  # collected on CPU; every test is skipped by the marker filter anyway
    ops = R = None

DEV = "cuda"


def require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# more than 2,048 rows exercises the grid-stride path (and its prefetch)
@pytest.mark.parametrize("C", [1024, 4096, 5120])
@pytest.mark.parametrize("rows", [1, 3, 257, 2049, 4100])
def test_fused_add_rmsnorm_reg_bit_identical(rows, C):
    require_gpu()
    g = torch.Generator(device=DEV).manual_seed(rows * 7 + C)
    x = torch.randn(rows, C, device=DEV, generator=g).bfloat16()
    res = (torch.randn(rows, C, device=DEV, generator=g) * 3).bfloat16()
    w = (torch.randn(C, device=DEV, generator=g) * 0.5 + 1.0).bfloat16()
    x0, r0 = x.clone(), res.clone()
    y0, nr0 = ops.fused_add_rmsnorm(x0, r0, w, 1e-6, variant="v1")
    x1, r1 = x.clone(), res.clone()
    y1, nr1 = ops.fused_add_rmsnorm(x1, r1, w, 1e-6, variant="reg")
    assert torch.equal(nr1, nr0)
    assert torch.equal(y1, y0)
    if rows == 257 and C == 5120:
        # and the pair is the op: against the fp32 reference
        ry, rr = R.fused_add_rmsnorm(x.cpu(), res.cpu(), w.cpu(), 1e-6)
        assert torch.allclose(y1.float().cpu(), ry.float(), atol=3e-2, rtol=3e-2)
        assert torch.allclose(nr1.float().cpu(), rr.float(), atol=3e-2, rtol=3e-2)
