"""TEST INFRASTRUCTURE: the one-bf16-ulp criterion the convolution tests hold a bf16 result to."""
import torch


def within_bf16_ulp(got_bf16, ref64):
    """|got - ref| <= 1 bf16 ulp of ref (+ 1e-5 max|ref| for values that cancel to ~0).  -> (ok, worst error in ulp)"""
    got = got_bf16.double().cpu()
    mag = ref64.abs().clamp_min(1e-30)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    err = (got - ref64).abs()
    return bool((err <= ulp + 1e-5 * float(ref64.abs().max())).all()), float((err / (ulp + 1e-30)).max())
