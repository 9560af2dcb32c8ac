"""Inputs that test_gpu_speed.py and test_gpu_stretch.py share: a configuration with extra keys, a noise bank, a pair of
views and a list of tracks, all from fixed seeds."""
import torch

from grafp_amd.util import load_config


def _cfg(**kw):
    return dict(load_config(), **kw)


def _noise_bank():
    return 0.1 * torch.randn(3, 20000, generator=torch.Generator().manual_seed(31))


def _views(B, L, dev, seed=6):
    g = torch.Generator().manual_seed(seed)
    x = 0.1 * torch.randn(B, L, generator=g)
    return x.to(dev), (x + 0.03 * torch.randn(B, L, generator=g)).to(dev)


def _tracks(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [0.2 * torch.randn(n, generator=g) for n in lengths]
