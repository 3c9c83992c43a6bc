"""CPU (emulator): the life cycle the four resident handles share — capi.ResidentHandle on the Python side, DimHandleBase's allocation list
and upload helpers (csrc/dim_common.h, api_ops.hip) on the C++ side: non-finite weights are rejected by every create, destroy runs at most
once, the allocator's byte accounting, and the stream helper resolves the current stream at every call.  One GPU test: calls issued on a side
stream give the bits of calls on the default stream."""
import importlib

import pytest
import torch

capi = importlib.import_module("deep-image-matching_amd.capi")
weights = importlib.import_module("deep-image-matching_amd.weights")
sp_hip = importlib.import_module("deep-image-matching_amd.superpoint_hip")
lg_hip = importlib.import_module("deep-image-matching_amd.lightglue_hip")
al_hip = importlib.import_module("deep-image-matching_amd.aliked_hip")
nn_hip = importlib.import_module("deep-image-matching_amd.nn_hip")


def _sp(lib, sd):
    return sp_hip.SuperPointHIP(sd, {}, max_hw=(16, 16), capacity=64, device="cpu", lib=lib)


def _sp_call(net):
    n = net.extract_batch(torch.rand(1, 16, 16, generator=torch.Generator().manual_seed(0)))[3]
    assert 0 <= int(n[0]) <= 64


def _lg(lib, sd):
    return lg_hip.LightGlueHIP(sd, {"n_layers": 1}, max_kpts=32, device="cpu", lib=lib)


def _lg_call(net):
    g = torch.Generator().manual_seed(0)
    kt, dt = torch.rand(2, 8, 2, generator=g) * 32, torch.nn.functional.normalize(torch.randn(2, 8, 256, generator=g), dim=-1)
    o = net.match_batch(kt.contiguous(), dt.contiguous(), torch.tensor([8, 8], dtype=torch.int32), torch.full((2, 2), 32.0), n_pairs=1)
    assert 0 <= int(o["n_matches"][0]) <= 8


def _al(lib, sd):
    return al_hip.AlikedHIP(sd, {"model_name": "aliked-t16", "max_num_keypoints": 64}, max_hw=(32, 32), device="cpu", lib=lib)


def _al_call(net):
    n = net.extract_batch(torch.rand(1, 32, 32, 3, generator=torch.Generator().manual_seed(0)))[3]
    assert 0 <= int(n[0]) <= 64


# (a): a tensor that goes to the device as fp32; (b): one whose matrix-core form is a split operand (a GEMM weight, a 3 x 3 convolution over >= 64 channels)
_CASES = {
    "superpoint": (lambda: weights.synthetic_superpoint_state_dict(0), _sp, _sp_call, "conv1a.bias", "conv3b.weight"),
    "lightglue": (lambda: weights.synthetic_lightglue_state_dict(0, n_layers=1), _lg, _lg_call, "posenc.Wr.weight", "transformers.0.self_attn.Wqkv.weight"),
    "aliked": (lambda: weights.synthetic_aliked_state_dict(7, "aliked-t16"), _al, _al_call, "block1.bn1.weight", "block4.conv2.regular_conv.weight"),
}


@pytest.fixture
def created(monkeypatch):
    """The wrapper objects whose constructor reached create, in order (a failing constructor leaves no other reference)."""
    seen, orig = [], capi.ResidentHandle._create

    def spy(self, *a):
        seen.append(self)
        return orig(self, *a)

    monkeypatch.setattr(capi.ResidentHandle, "_create", spy)
    return seen


@pytest.mark.parametrize("which", sorted(_CASES))
def test_every_create_rejects_non_finite_weights(emu_lib, created, which):
    make_sd, make, call, key_f32, key_split = _CASES[which]
    sd = make_sd()
    for key in (key_f32, key_split):
        bad = dict(sd)
        t = bad[key].clone()
        t.view(-1)[t.numel() // 2] = float("nan")
        bad[key] = t
        with pytest.raises(capi.DimHipError, match="non-finite"):
            make(emu_lib, bad)
        obj = created.pop()
        assert not obj._h     # null, and __del__ (twice: the interpreter's comes on top) has nothing to do
        obj.__del__()
    net = make(emu_lib, sd)   # the library is as usable as before
    assert net._h
    call(net)


def test_destroy_is_called_at_most_once(emu_lib, created):
    capi.declare_nn(emu_lib)
    calls = []
    real = emu_lib.dim_nn_destroy
    emu_lib.dim_nn_destroy = lambda h: calls.append(h) or real(h)
    try:
        net = nn_hip.NearestNeighborHIP(max_pairs=1, max_kpts=64, dim=64, device="cpu", lib=emu_lib)
        assert net._h
        net.__del__()
        assert len(calls) == 1 and not net._h
        net.__del__()
        del net    # the interpreter's own call comes on top
        assert len(calls) == 1
        calls.clear()
        with pytest.raises(capi.DimHipError, match="multiple of 64"):
            nn_hip.NearestNeighborHIP(max_pairs=1, max_kpts=64, dim=65, device="cpu", lib=emu_lib)
        obj = created.pop()
        assert not obj._h
        obj.__del__()
        del obj
        assert calls == []
    finally:
        del emu_lib.dim_nn_destroy


def test_nn_workspace_bytes_are_the_requested_bytes(emu_lib):
    """dim_nn_create (nn_match.hip) with P pairs, NK = max_kpts rounded up to 4, T = ceil(NK / 128) tiles, 4-byte elements:
    owner 2 P + norms 2 P NK + rp P T 3 NK + cp P T 3 NK + fin P 2 3 NK = 4 (4 + 400 + 600 + 600 + 1200) for P = 2, NK = 100, T = 1 — the value the
    library returned before the allocator moved into DimHandleBase: the per-allocation slack is not counted."""
    net = nn_hip.NearestNeighborHIP(max_pairs=2, max_kpts=100, dim=64, device="cpu", lib=emu_lib)
    assert net.workspace_bytes() == 11216


def test_stream_ptr_resolves_the_current_stream_at_every_call(monkeypatch):
    class _Stream:
        def __init__(self, v):
            self.cuda_stream = v

    streams = iter([_Stream(0x1000), _Stream(0x2000)])
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: next(streams))
    dev = torch.device("cuda", 0)
    a, b = capi.stream_ptr(dev), capi.stream_ptr(dev)
    assert (a.value, b.value) == (0x1000, 0x2000)
    assert capi.stream_ptr("cpu") is None


@pytest.mark.gpu
def test_calls_on_a_side_stream_give_the_bits_of_the_default_stream(hip_lib):
    """SuperPoint at 64 x 64 and the NN matcher on 64 x 64 descriptors of width 64, once on the default stream and once inside
    torch.cuda.stream(side): a wrong stream or device context in the wrapper base shows as a race or as outputs read before the kernels ran."""
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(3)
    img = torch.rand(1, 64, 64, generator=g).to(dev)
    desc = torch.nn.functional.normalize(torch.randn(2, 64, 64, generator=g), dim=-1).to(dev).contiguous()
    cnt = torch.tensor([64, 64], dtype=torch.int32, device=dev)
    sp = sp_hip.SuperPointHIP(weights.synthetic_superpoint_state_dict(0), {"max_keypoints": 128}, max_hw=(64, 64), device=dev)
    nn = nn_hip.NearestNeighborHIP("mnn", 0.9, dim=64, max_pairs=1, max_kpts=64, device=dev)

    def both():
        e = sp.extract_batch(img)
        m = nn.match_batch(None, desc, cnt, n_pairs=1)
        return list(e) + [m["matches"], m["scores"], m["n_matches"]]

    torch.cuda.synchronize(dev)
    want = both()
    torch.cuda.synchronize(dev)
    want = [t.cpu() for t in want]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        assert sp._stream().value == side.cuda_stream
        got = both()
    side.synchronize()
    got = [t.cpu() for t in got]
    k, S = int(want[3][0]), int(want[6][0])
    assert k > 0 and S > 0
    assert int(got[3][0]) == k and int(got[6][0]) == S
    for w, g_, n in ((want[0], got[0], k), (want[1], got[1], k), (want[2], got[2], k)):
        assert torch.equal(w[0, :n], g_[0, :n])
    assert torch.equal(want[4][0, :S], got[4][0, :S]) and torch.equal(want[5][0, :S], got[5][0, :S])
