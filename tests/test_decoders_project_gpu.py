"""The FPN decoders in the projected form (kpfpn._decoder: the coarse level goes through its part of the Linear BEFORE it is
up-sampled, the skip GEMM adds the projected rows by index) against the concat form (COFI_DECODER_CONCAT=1) and a CPU fp64 evaluation of
kp_backbone.py:111-124, on a small synthetic stack-mode pyramid in the flagship arithmetic.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# points per frame: the smallest synthetic frame the suite runs end to end (the driver's smoke run) - its coarsest stage still has the
# 128 points a neighbour table row needs, and every stage is a whole number of 64-row statistics slabs per frame, which stack mode requires
NUM_POINTS = 2048
DEC = (("decoder4", 3, 2048), ("decoder3", 2, 1024), ("decoder2", 1, 512))   # name, stage of its rows, columns from the coarser level


def _pyramid(frames):
    from cofii2p_amd.network import CoFiI2P
    from cofii2p_amd.preprocess import build_pyramid
    from cofii2p_amd.synth import make_frame, subsample_indices

    pyrs = []
    for fid in range(frames):
        fr = make_frame(90 + fid, NUM_POINTS)
        sub = [torch.from_numpy(s).to(DEV) for s in subsample_indices(NUM_POINTS, 5, seed=90 + fid)]
        pyr = build_pyramid(torch.from_numpy(fr.points).to(DEV), sub)
        pyr["feats"] = torch.from_numpy(fr.feats).to(DEV)
        pyrs.append(pyr)
    img = torch.zeros(1, 3, 8, 8, device=DEV)
    return CoFiI2P.stack_frames(pyrs, [img] * frames)[0]


def _model(norm):
    from cofii2p_amd.network import CoFiI2P

    class Opt:
        img_H, img_W, img_fine_resolution_scale = 160, 512, 32

    Opt.norm = norm
    return CoFiI2P(Opt(), arithmetic="bf16x6").to(DEV).eval()


def _w(P, key):
    v = P[key]
    return (v.w if hasattr(v, "w") else v).double().cpu()


def _decoder_fp64(P, kind, name, coarse, stage, idx, frames):
    """kp_backbone.py:111-124 in fp64: Linear over cat[nearest_upsample(coarse), stage], then the encoder's normalisation + LeakyReLU(0.1)
    (decoder2: the Linear alone).  'bn': the packed weights already hold the folded BatchNorm."""
    p = "pc_encoder.%s." % name
    rows, crow = stage.shape[0] // frames, coarse.shape[0] // frames
    up = []
    for f in range(frames):
        pad = torch.cat([coarse[f * crow:(f + 1) * crow], torch.zeros(1, coarse.shape[1], dtype=torch.float64)], 0)   # shadow row
        up.append(pad[idx[f * rows:(f + 1) * rows].long().clamp(0, crow)])
    y = torch.cat([torch.cat(up, 0), stage], 1) @ _w(P, p + "mlp.weight").t() + _w(P, p + "mlp.bias")
    if name == "decoder2":
        return y
    if kind == "gn":
        y = torch.cat([torch.nn.functional.group_norm(y[f * rows:(f + 1) * rows].t()[None], 32, _w(P, p + "norm.norm.weight"),
                                                      _w(P, p + "norm.norm.bias"), 1e-5)[0].t() for f in range(frames)], 0)
    elif kind == "ln":
        y = torch.nn.functional.layer_norm(y, (y.shape[1],), _w(P, p + "norm.weight"), _w(P, p + "norm.bias"), 1e-5)
    return torch.nn.functional.leaky_relu(y, 0.1)


@pytest.mark.parametrize("norm,frames", [("gn", 2), ("bn", 1), ("ln", 1)])
def test_projected_decoders_match_concat_form(norm, frames, monkeypatch):
    """Per decoder: the largest absolute error of both forms against fp64 (computed from the encoder outputs of the run under test);
    the projected form may be at most 2 x the concat form's + 1e-7 max|reference| - one extra fp32 rounding from adding two separately
    accumulated sums.  The projected form launches no cofi_gather_rows, the concat form its three."""
    from cofii2p_amd import kpfpn, ops

    m = _model(norm)
    P = m._pack(torch.device(DEV))
    kind = P["pc_encoder.__norm__"]
    assert kind == norm
    data = _pyramid(frames)
    up_idx = [t[:, 0].cpu() for t in data["upsampling"]]
    calls = []
    real = ops.gather_rows
    monkeypatch.setattr(ops, "gather_rows", lambda *a, **k: (calls.append(a[0].shape), real(*a, **k))[1])
    monkeypatch.setattr(kpfpn, "DECODER_PROJECT_MIN_ROWS", {})   # every decoder in the projected form, whatever its row count
    err, scale = {}, {}
    with torch.no_grad(), ops.arithmetic("bf16x6"):
        for form in ("projected", "concat"):
            monkeypatch.setattr(kpfpn, "DECODER_CONCAT", form == "concat")
            del calls[:]
            taps = {}
            kpfpn.run_fpn(P, data["points"], data["neighbors"], data["subsampling"], data["upsampling"], data["feats"], taps=taps, frames=frames)
            torch.cuda.synchronize()
            assert len(calls) == (3 if form == "concat" else 0), (form, calls)
            stage = {1: taps["encoder2_3"], 2: taps["encoder3_3"], 3: taps["encoder4_3"]}
            coarse = taps[[b.name for b in kpfpn.ENCODER if b.stage == 4][-1]].double().cpu()
            for name, st, upc in DEC:
                assert P["pc_encoder.%s.mlp.up.weight" % name].shape[1] == upc
                ref = _decoder_fp64(P, kind, name, coarse, stage[st].double().cpu(), up_idx[st], frames)
                err[form, name] = float((taps[name].double().cpu() - ref).abs().max())
                scale[name] = float(ref.abs().max())
                coarse = ref   # the fp64 chain: the next decoder's coarse level
    report = "; ".join("%s: projected %.3e, concat %.3e (max|ref| %.2f)" % (n, err["projected", n], err["concat", n], scale[n]) for n, _, _ in DEC)
    print("decoder errors against fp64 [%s, %d frame(s)] %s" % (norm, frames, report))
    for name, _, _ in DEC:
        assert err["projected", name] <= 2.0 * err["concat", name] + 1e-7 * scale[name], (norm, report)

