"""The image-quality pipeline restated in torch on the CPU, in fp64 or fp32 (METRICS.md): the z-score, torchvision's vgg16().features
layout (64 64 M 128 128 M 256 256 256 M 512 512 512 M 512 512 512, the last pool never reached), the LPIPS tap, PSNR and SSIM."""
import math

import torch
import torch.nn.functional as F

MEAN = (-.030, -.088, -.188)
STD = (.458, .448, .450)
TAP_AFTER = (1, 3, 6, 9, 12)
POOL_AFTER = (1, 3, 6, 9)


def T(a, dtype=torch.float64):
    return torch.as_tensor(a).to(dtype)


def z_score(x, dtype):
    """networks.py:41-51; mean and std are fp32 buffers there, so they enter fp64 as the fp32 values."""
    m = torch.tensor(MEAN, dtype=torch.float32).to(dtype)[None, :, None, None]
    s = torch.tensor(STD, dtype=torch.float32).to(dtype)[None, :, None, None]
    return (x - m) / s


def conv_relu(x, w, b):
    return F.relu(F.conv2d(x, w, b, padding=1))


def conv_abs(x, w, b):
    """sum |a . b| per output value, the bias included: the scale of the rounding bound of a k-ordered fma chain."""
    return F.conv2d(x.abs(), w.abs(), b.abs(), padding=1)


def pool(x):
    return F.max_pool2d(x, 2, 2)


def features(x, convs, biases, dtype=torch.float64):
    """The five tapped feature maps [1, C, h, w] of x [1, 3, H, W] (before normalisation)."""
    x = z_score(T(x, dtype), dtype)
    out = []
    for k, (w, b) in enumerate(zip(convs, biases)):
        x = conv_relu(x, T(w, dtype), T(b, dtype))
        if k in TAP_AFTER:
            out.append(x)
        if k in POOL_AFTER:
            x = pool(x)
    return out


def tap(fx, fy, lin):
    """modules/utils.py:6-8 and modules/lpips.py:33-34 for one layer: a scalar tensor."""
    nx = torch.sqrt(torch.sum(fx ** 2, 1, keepdim=True))
    ny = torch.sqrt(torch.sum(fy ** 2, 1, keepdim=True))
    d = (fx / (nx + 1e-10) - fy / (ny + 1e-10)) ** 2
    return (d * lin.reshape(1, -1, 1, 1).to(d.dtype)).sum(1).mean()


def lpips(x, y, weights, dtype=torch.float64):
    """{"features": (fx, fy), "terms": [5] tensor, "total": scalar tensor} for x, y [1, 3, H, W] or [3, H, W]."""
    convs, biases, lins = weights
    x, y = T(x, dtype).reshape(1, 3, *x.shape[-2:]), T(y, dtype).reshape(1, 3, *y.shape[-2:])
    fx, fy = features(x, convs, biases, dtype), features(y, convs, biases, dtype)
    terms = torch.stack([tap(a, b, T(l, dtype)) for a, b, l in zip(fx, fy, lins)])
    total = terms[0]
    for k in range(1, 5):
        total = total + terms[k]
    return {"features": (fx, fy), "terms": terms, "total": total}


def mse(x, y, dtype=torch.float64):
    x, y = T(x, dtype), T(y, dtype)
    return ((x - y) ** 2).reshape(x.shape[0], -1).mean(1, keepdim=True)


def psnr(x, y, dtype=torch.float64):
    return 20 * torch.log10(1.0 / torch.sqrt(mse(x, y, dtype)))


def ssim(x, y, dtype=torch.float64, window_size=11):
    """utils/loss_utils.py:43-73, size_average=True; the window is built in fp32 there (create_window's .float())."""
    x, y = T(x, dtype).reshape(1, 3, *x.shape[-2:]), T(y, dtype).reshape(1, 3, *y.shape[-2:])
    g = torch.Tensor([math.exp(-(i - window_size // 2) ** 2 / float(2 * 1.5 ** 2)) for i in range(window_size)])
    g = (g / g.sum()).unsqueeze(1)
    window = g.mm(g.t()).float().unsqueeze(0).unsqueeze(0).expand(3, 1, window_size, window_size).contiguous().to(dtype)
    conv = lambda a: F.conv2d(a, window, padding=window_size // 2, groups=3)
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = conv(x * x) - mu1_sq
    s2 = conv(y * y) - mu2_sq
    s12 = conv(x * y) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m.mean()
