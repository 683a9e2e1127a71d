"""Where the one-pass variance of GroupNorm and BatchNorm (E[x^2] - E[x]^2 from fp32 sums) stops being bf16-accurate: the relative
rstd error of nk_groupnorm_fwd and nk_batchnorm_fwd against float64 as the mean moves away from zero, at the UNet's 128^2-latent
GroupNorm (batch 4, 320 channels: 163 840 elements per group) and the PatchGAN's BatchNorm at M = 131 072.  Half a bf16 ulp is
2^-9 = 1.95e-3 relative.

    python tools/norm_one_pass_limit.py
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402


def main():
    from neurosis_amd import ops

    F64 = torch.float64
    print(f"{'|mean|/sigma':>12} {'GroupNorm rstd':>15} {'BatchNorm rstd':>15}   (max relative error against float64; half a bf16 ulp = 1.95e-3)")
    for ratio in (0, 8, 16, 32, 64, 128):
        g = torch.Generator(device="cuda").manual_seed(ratio)
        # GroupNorm: N = 4, 128 x 128, C = 320, G = 32; each group's mean at +-ratio sigma
        N, HW, C, G = 4, 128 * 128, 320, 32
        sign = (((torch.arange(C, device="cuda") // (C // G)) % 2) * 2 - 1).float()
        x = (torch.randn(N * HW, C, generator=g, device="cuda") + ratio * sign).to(torch.bfloat16)
        w, b = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        y = torch.empty_like(x)
        mean, rstd = (torch.empty(N, G, device="cuda") for _ in range(2))
        ws = ops._ws(ops.query("nk_groupnorm_ws_floats", N, HW, C, G), x.device)
        ops.call("nk_groupnorm_fwd", x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(),
                 N, HW, C, G, 1e-5, 0, ops._stream())
        xd = x.to(F64).view(N, HW, G, C // G)
        ref = (xd.var((1, 3), unbiased=False) + 1e-5).rsqrt()
        gn = float(((rstd.to(F64) - ref).abs() / ref).max())
        # BatchNorm: M = 131 072, C = 128; each channel's mean at +-ratio sigma
        M, C = 131072, 128
        sign = torch.where(torch.arange(C, device="cuda") % 2 == 0, 1.0, -1.0)
        x = (torch.randn(M, C, generator=g, device="cuda") + ratio * sign).to(torch.bfloat16)
        w, b = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        y = torch.empty_like(x)
        mean, rstd = (torch.empty(C, device="cuda") for _ in range(2))
        ws = ops._ws(ops.query("nk_batchnorm_ws_floats", M, C), x.device)
        ops.call("nk_batchnorm_fwd", x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None, None,
                 ws.data_ptr(), M, C, 1e-5, 0.1, 1.0, ops._stream())
        ref = (x.to(F64).var(0, unbiased=False) + 1e-5).rsqrt()
        bn = float(((rstd.to(F64) - ref).abs() / ref).max())
        print(f"{ratio:>12} {gn:>15.3e} {bn:>15.3e}")


if __name__ == "__main__":
    main()
