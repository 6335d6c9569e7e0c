"""The width-128 forward's ReLUs (csrc/mlp128_chain32.h: relu, relu_block,
relu_values) through psvo_mlp_fwd: the stored masks against the stored
activations, the activations' bits at the edge values (±0, denormals, large),
the value-only trunk (k_mlp_sdf2) against the training forward, and the
engine's interpolating trunk against the two kernels it replaces.  Everything
is compared as int32 bit patterns."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_trunk_interp import _run as trunk_run
from test_gpu_trunk_interp import case  # noqa: F401  (the small case's builder: a module fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"

# one partial unit, a unit + 1, a 256-sample tile + 1, several rounds of the persistent loop
SIZES = [1, 33, 257, 2049]
EDGE = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-38, 1.0, -1.0, 3e38, -3e38], dtype=np.float32)
NEG_ZERO = np.int32(-2 ** 31)


def _random_decoder():
    from psvo.decoder import Decoder
    torch.manual_seed(3)
    dec = Decoder(depth=2, width=128, in_dim=16, skips=[], embedder="none")
    return [p.detach().float().contiguous() for p in dec.fused_params()]


def _edge_decoder():
    """The random decoder with a first layer that passes chosen features
    through: row i of W1 is +1 or −1 on input i % 16 (sign by (i / 16) % 2),
    b1[i] is +0.0 or −0.0 (by (i / 32) % 2).  The later layers are scaled down
    so that h1 = 3e38 does not overflow them."""
    ps = _random_decoder()
    i = torch.arange(128)
    w1 = torch.zeros(128, 16)
    w1[i, i % 16] = torch.where((i // 16) % 2 == 0, 1.0, -1.0)
    b1 = torch.where((i // 32) % 2 == 0, 0.0, -0.0).float()
    assert int((b1.view(torch.int32) == int(NEG_ZERO)).sum()) == 64
    ps[0], ps[1] = w1, b1
    for k in (2, 4, 6):
        ps[k] = ps[k] * 0.01
    return ps


def _edge_feat(m):
    s = np.arange(m)[:, None]
    k = np.arange(16)[None, :]
    return EDGE[(s + 2 * k) % len(EDGE)]  # every value on every input within 9 samples


def _random_feat(m):
    g = torch.Generator().manual_seed(11)
    return (torch.randn(m, 16, generator=g) * 0.5).numpy()


DECODERS = {"random": (_random_decoder, _random_feat), "edge": (_edge_decoder, _edge_feat)}


@functools.lru_cache(maxsize=None)
def _forward(which, m):
    """One training call (act + masks) and one sdf-only call of psvo_mlp_fwd on
    the same inputs, computed once per (decoder, m) and shared; host int32 /
    int64 arrays: sdf, rgb, act [4][tiles][128][32] (CF order), masks [m][2][3],
    the sdf-only call's sdf, and the inputs."""
    from psvo import _lib as L
    make_dec, make_feat = DECODERS[which]
    ps_host = make_dec()
    ps = [p.to(DEV) for p in ps_host]
    feat_host = np.ascontiguousarray(make_feat(m), dtype=np.float32)
    feat = torch.from_numpy(feat_host).to(DEV)
    lib = L.lib()
    images = torch.empty(int(lib.psvo_mlp_image_floats_w(128)), dtype=torch.float32, device=DEV)
    n_act = int(lib.psvo_mlp_act_floats(m, 128))
    act = torch.full((n_act,), float("nan"), dtype=torch.float32, device=DEV)
    masks = torch.full((int(lib.psvo_mlp_mask_words(m, 128)),), -1, dtype=torch.int64, device=DEV)
    sdf = torch.empty(m, dtype=torch.float32, device=DEV)
    rgb = torch.empty((m, 3), dtype=torch.float32, device=DEV)
    L.call("psvo_mlp_fwd", L.stream_of(DEV), m, 128, feat, *ps, images, sdf, rgb, act, masks)
    sdf_only = torch.empty(m, dtype=torch.float32, device=DEV)
    L.call("psvo_mlp_fwd", L.stream_of(DEV), m, 128, feat, *ps, images, sdf_only, None, None, None)
    torch.cuda.synchronize()
    assert n_act % (4 * 4096) == 0 and n_act // (4 * 4096) >= (m + 31) // 32
    return {
        "sdf": sdf.view(torch.int32).cpu().numpy(), "rgb": rgb.cpu().numpy(),
        "act": act.view(torch.int32).cpu().numpy().reshape(4, -1, 128, 32),
        "masks": masks.cpu().numpy().reshape(m, 2, 3),
        "sdf_only": sdf_only.view(torch.int32).cpu().numpy(),
        "feat": feat_host, "w1": ps_host[0].numpy(), "b1": ps_host[1].numpy(),
    }


def _rows(act, layer, m):
    """Layer `layer` (0 h1, 1 h2, 2 f, 3 c1) of the CF activations as [m][128]
    int32: per 32-sample tile a [128][32] block, tile-local sample c at
    position p = 16 (c & 1) + c / 2, the row's 16-B groups XOR-ed by (f / 2) % 8
    (csrc/mlp128.h)."""
    s = np.arange(m)[:, None]
    f = np.arange(128)[None, :]
    c = s % 32
    p = 16 * (c & 1) + c // 2
    slot = (((p >> 2) ^ ((f // 2) % 8)) << 2) | (p & 3)
    return act[layer][s // 32, f, slot]


def _mask_bits(masks, word, m):
    """Mask word `word` (0 m1, 1 m2, 2 m4) as [m][128] booleans: feature
    32 b + phi(r, h) is bit 16 b + r of lane half h's word, phi(r, h) =
    (r & 3) + 8 (r >> 2) + 4 h."""
    f = np.arange(128)
    b, ff = f >> 5, f & 31
    h = (ff >> 2) & 1
    r = (ff & 3) + 4 * (ff >> 3)
    w = masks[:, :, word].astype(np.uint64)  # [m][2]
    return ((w[:, h] >> (16 * b + r).astype(np.uint64)) & np.uint64(1)).astype(bool)


@pytest.mark.parametrize("which", ["random", "edge"])
@pytest.mark.parametrize("m", SIZES)
def test_masks_agree_with_stored_activations(which, m):
    """h1, h2 and c1: every mask bit equals (stored activation > 0) of the same
    call; every stored activation is >= 0 and none is −0.0 (ReLU writes +0.0
    for every non-positive input)."""
    out = _forward(which, m)
    for layer, word, name in ((0, 0, "h1"), (1, 1, "h2"), (3, 2, "c1")):
        a = _rows(out["act"], layer, m)
        bits = _mask_bits(out["masks"], word, m)
        val = a.view(np.float32)
        print(f"{which} m={m} {name}: {int(bits.sum())} of {bits.size} on, "
              f"{int((a == 0).sum())} stored +0.0, {int((a == NEG_ZERO).sum())} stored -0.0, "
              f"{int((bits != (val > 0)).sum())} mask bits differ")
        assert not (a == NEG_ZERO).any(), name
        assert (a >= 0).all(), name  # sign bit clear: >= +0.0, no negative value or NaN
        assert np.array_equal(bits, val > 0), name
        assert 0 < int(bits.sum()) < bits.size, name  # both outcomes occur


@pytest.mark.parametrize("m", SIZES)
def test_edge_values_reach_the_relu(m):
    """The pass-through first layer: pre = ±x + b1 with one non-zero product per
    row, so the host knows it exactly (where x is ±0 the sum is a zero of either
    sign: ReLU gives +0.0 for both).  Pre-activations of ±0, ± denormal, ±1 and
    ±3e38 all occur; h1 is bit-equal to max(pre, 0) with +0.0 for every
    non-positive pre, and mask bit = (pre > 0)."""
    out = _forward("edge", m)
    f = np.arange(128)
    sign = out["w1"][f, f % 16]
    pre = (sign[None, :] * out["feat"][:, f % 16]).astype(np.float32)
    want = np.where(pre > 0, pre, np.float32(0.0)).astype(np.float32)
    h1 = _rows(out["act"], 0, m)
    bits = _mask_bits(out["masks"], 0, m)
    tiny = np.float32(1.1754944e-38)
    n_den = int(((pre > 0) & (pre < tiny)).sum())
    print(f"m={m}: pre > 0 {int((pre > 0).sum())}, positive denormal {n_den}, zero {int((pre == 0).sum())}, "
          f"h1 bits differ {int((h1 != want.view(np.int32)).sum())}, mask bits differ {int((bits != (pre > 0)).sum())}")
    if m >= len(EDGE):
        for v in EDGE[EDGE != 0]:
            assert (pre == v).any() and (pre == -v).any(), v
        assert n_den > 0
    assert np.array_equal(h1, want.view(np.int32))
    assert np.array_equal(bits, pre > 0)


@pytest.mark.parametrize("which", ["random", "edge"])
@pytest.mark.parametrize("m", SIZES)
def test_sdf_only_forward_equals_full_forward(which, m):
    """rgb == NULL (k_mlp_sdf2: value-only ReLUs) gives the training call's
    sdf (k_mlp_fwd2: ReLUs with masks), bit for bit."""
    out = _forward(which, m)
    assert np.array_equal(out["sdf_only"], out["sdf"])
    assert np.isfinite(out["sdf"].view(np.float32)).all()
    assert np.isfinite(out["rgb"]).all()


def test_engine_trunk_matches_interp_pass_then_plain_trunk(case):  # noqa: F811
    """The mapping step's device-sized trunk (k_mlp_sdf2<true, true>) on every
    sample of the small case: sdf, h2 rows and feature rows bit-equal to the
    interpolation pass followed by the plain trunk (k_mlp_sdf2<false, false>),
    and the h2 rows are ReLU outputs (>= +0.0, never −0.0)."""
    c = case
    n = c["m"]
    two = trunk_run(c, 0, n, c["m_cap"])
    one = trunk_run(c, 1, n, c["m_cap"])
    for name, a, b in zip(("sdf", "h2", "feat"), one, two):
        assert torch.equal(a[:n], b[:n]), name
    assert torch.equal(one[2][:n], c["feat_ref"][:n])
    assert bool((one[1][:n] >= 0).all())
    assert 0 < int((one[1][:n] > 0).sum()) < one[1][:n].numel()
