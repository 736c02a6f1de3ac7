"""The tile-offset scan between the count and emit launches of K10 and K15 (csrc/scan.hip) on
the MI355X, on its own: exact against ``torch.cumsum`` in int64.  One workgroup of 256 lanes
scans all tiles, so the sizes run from no tile over fewer tiles than lanes (the trailing lanes
own none) to several tiles per lane."""
import pytest
import torch

from analyzer_amd.ops.native import native

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 255, 256, 257, 1000, 70001]


def check_offsets(counts, device):
    """counts: int64 [T] in [0, 2^32); the kernel reads them as the words of an int32 tensor."""
    T = counts.numel()
    words = torch.where(counts >= 1 << 31, counts - (1 << 32), counts).to(torch.int32)
    offsets = native().tile_offsets(words.to(device))
    assert offsets.is_cuda and offsets.dtype == torch.int64 and tuple(offsets.shape) == (T + 1,)
    got = offsets.cpu()
    want = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])
    assert int(got[0]) == 0 and int(got[T]) == int(counts.sum())
    assert torch.equal(got, want), (T, (got != want).nonzero().reshape(-1)[:5].tolist())


@pytest.mark.parametrize("T", SIZES)
def test_tile_offsets_random_counts(gpu_device, T):
    g = torch.Generator().manual_seed(1000 + T)
    check_offsets(torch.randint(0, 1 << 32, (T,), generator=g, dtype=torch.int64), gpu_device)
    check_offsets(torch.randint(0, 5000, (T,), generator=g, dtype=torch.int64), gpu_device)  # what a tile can hold


def test_tile_offsets_total_beyond_32_bits(gpu_device):
    """Every count 0xF0000000: a lane's own partial sum passes 2^32 already, so the sums are
    64-bit from the first addition on."""
    T = SIZES[-1]
    check_offsets(torch.full((T,), 0xF0000000, dtype=torch.int64), gpu_device)
    assert T * 0xF0000000 > 1 << 32
