"""32 query rows per wave on short sequences (Sq <= 512, Sq % 128 == 0, at least TANGO_ATTN_QB2_MIN_WGS workgroups): the product path of
level-2 self-attention at B >= 8 and of level 3 of 20-s clips, which no op test reaches at the default of 512 workgroups.  The smallest
shapes of the branch -- one and two 128-row blocks, and the 64-key cross form with a key mask -- with the threshold lowered to one
workgroup, against the full fp64 reference (reference op: attention_processor.py:495-540)."""
import ctypes as C

import pytest
import torch

from test_attention_defer_gpu import TOL
from test_duo_gpu import tuning
from test_ops_gpu import close, quant

pytestmark = pytest.mark.gpu

DT = {"fp32": 0, "fp16": 1, "bf16": 2}


@pytest.mark.parametrize("dtype", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("B,heads,Sq,Skv,masked", [(2, 3, 128, 128, False), (2, 3, 256, 256, False), (2, 2, 256, 64, True)])
def test_attention_short_sequences_at_32_rows_per_wave(lib, dtype, B, heads, Sq, Skv, masked):
    g = torch.Generator().manual_seed(Sq + Skv)
    C_ = heads * 64
    q = quant(torch.randn(B, Sq, C_, generator=g), dtype)
    k = quant(torch.randn(B, Skv, C_, generator=g), dtype)
    v = quant(torch.randn(B, Skv, C_, generator=g), dtype)
    bias = None
    if masked:
        m = torch.ones(B, Skv)
        m[0, 1:] = 0
        m[1, Skv // 2:] = 0
        bias = (1 - m) * -10000.0
    qh, kh, vh = (t.view(B, -1, heads, 64).transpose(1, 2).double() for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * 0.125
    if bias is not None:
        s = s + bias.double()[:, None, None, :]
    ref = (s.softmax(-1) @ vh).transpose(1, 2).reshape(B, Sq, C_)
    out = torch.empty(B, Sq, C_, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    qd, kd, vd, bd = q.cuda(), k.cuda(), v.cuda(), bias.cuda() if masked else None
    with tuning(lib, TANGO_ATTN_QB2_MIN_WGS=1):
        route = lib.tango_debug_attention_route(DT[dtype], B, heads, Sq, Skv, int(masked), 0, 0, 0).decode()
        rc = lib.tango_op_attention(DT[dtype], p(qd), p(kd), p(vd), p(bd), p(out), B, heads, Sq, Skv, C.c_float(0.125), None)
    assert rc == 0, lib.tango_last_error().decode()
    assert route.startswith("qb2:"), route
    if dtype == "fp32":
        close(out, ref, dtype, "attention " + route)
    else:
        err = (out.cpu() - ref.float()).abs().max().item() / ref.abs().max().item()
        print("attention %s B=%d h=%d Sq=%d Skv=%d %s: vs fp64 %.3e" % (dtype, B, heads, Sq, Skv, route, err))
        assert err <= TOL[dtype], (route, err)
