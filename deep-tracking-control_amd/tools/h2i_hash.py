"""Digest of the image-operand GEMM results on fixed operands (forward image + fp32 + sign record, data gradient with and without a sign
record, several operand images, the fused MSE layer): run under two builds (DTC_LIB) to check that a kernel variant is bit-identical."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dtc_amd import h2i, ops  # noqa: E402

DEV = "cuda:0"
g = torch.Generator(device=DEV).manual_seed(7)


def digest(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def rows(M, K):
    return torch.randn(M, K, device=DEV, generator=g) * torch.exp(3 * torch.randn(M, 1, device=DEV, generator=g))


# the large shapes of the step, then the small ones: 1, 2, 3, 4, 5, 8, 9, 10, 17, 65 and 128 stages of the reduction (M = 200: a partly
# empty row tile; N = 140: a partly empty column tile), 64 / 128 result columns where a sign record exists
SHAPES = ((24576, 512, 512), (24576, 693, 512), (4096, 512, 752), (777, 256, 584),
          (200, 140, 5), (200, 128, 16), (64, 140, 32), (200, 128, 48), (200, 64, 64), (200, 140, 80), (64, 128, 128), (200, 140, 144),
          (200, 128, 160), (200, 140, 272), (200, 128, 1040), (200, 140, 2048), (24576, 512, 256), (24576, 128, 64), (24576, 12, 128))
for M, N, K in SHAPES:
    X = rows(M, K)
    W, b = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5, torch.randn(N, device=DEV, generator=g)
    Xi, Yi, wset = h2i.HImage.from_tensor(X), h2i.HImage(M, N, DEV), h2i.WeightSet()
    Y = torch.empty(M, N, device=DEV)
    big = M >= 777 and N >= 256
    mask = ops.relu_mask(M, N, DEV).zero_() if ((N % 128 == 0 and M % 128 == 0) if big else ops.relu_mask_ok(M, N)) else None
    h2i.linear_fwd(Xi, W, b, Y, Yi, "relu" if mask is not None else None, mask=mask, wset=wset)
    dZi, dXi = h2i.HImage.from_tensor(torch.randn(M, N, device=DEV, generator=g)), h2i.HImage(M, K, DEV)
    dX = torch.empty(M, K, device=DEV)
    h2i.linear_dgrad(dZi, W, dX, dXi, mask=None, wset=wset)
    out = [Y, Yi.to_tensor(), dX, dXi.to_tensor()]
    if not big:
        out += [Yi.buf] + ([mask] if mask is not None else [])
    print(M, N, K, digest(*out))

# data gradient through a sign record (the record of a ReLU layer with `K` outputs, written by the forward kernel), reduction N
for M, N, K in ((24576, 512, 512), (24576, 256, 512), (200, 64, 128), (200, 12, 128), (200, 272, 64), (200, 2048, 128)):
    pre = torch.randn(M, K, device=DEV, generator=g)
    mask = ops.relu_mask(M, K, DEV).zero_()
    h2i.linear_fwd(h2i.HImage.from_tensor(pre), torch.eye(K, device=DEV), None, None, h2i.HImage(M, K, DEV), "relu", mask=mask)
    W = torch.randn(N, K, device=DEV, generator=g) / N ** 0.5
    dX, dXi = torch.empty(M, K, device=DEV), h2i.HImage(M, K, DEV)
    h2i.linear_dgrad(h2i.HImage.from_tensor(rows(M, N)), W, dX, dXi, mask=mask)
    print("dgrad+record", M, N, K, digest(dX, dXi.buf))

# several operand images (side by side), and the fused MSE layer
for M, N, widths in ((24576, 512, (512, 53, 19)), (200, 64, (19, 512)), (200, 140, (19, 512, 19))):
    imgs = [h2i.HImage.from_tensor(rows(M, w)) for w in widths]
    W, b = torch.randn(N, sum(widths), device=DEV, generator=g) / 23, torch.randn(N, device=DEV, generator=g)
    Y, Yi = torch.empty(M, N, device=DEV), h2i.HImage(M, N, DEV)
    h2i.linear_fwd(imgs, W, b, Y, Yi, "elu")
    print("images", M, N, widths, digest(Y, Yi.buf))
for M, N, K in ((24576, 693, 512), (200, 140, 80)):
    X, W, b = rows(M, K), torch.randn(N, K, device=DEV, generator=g) / K ** 0.5, torch.randn(N, device=DEV, generator=g)
    T = torch.randn(2 * M, 1389, device=DEV, generator=g)
    idx = torch.randint(0, 2 * M, (M,), device=DEV, generator=g)
    dY, dYi = torch.empty(M, N, device=DEV), h2i.HImage(M, N, DEV)
    part = torch.zeros(h2i.mse_parts(M, N), dtype=torch.float64, device=DEV)
    n = h2i.linear_fwd_mse(h2i.HImage.from_tensor(X), W, b, T, 696, idx, dY, dYi, part)
    print("mse", M, N, K, digest(dY, dYi.buf, part[:n]))
