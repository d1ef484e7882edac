"""pack_encoder's column split of the decoder weights (kpfpn.DECODER_UP): no GPU needed."""
import numpy as np
import torch

DEC = (("decoder4", 2048, 3072, 1024), ("decoder3", 1024, 1536, 512), ("decoder2", 512, 768, 64))   # name, up columns, inputs, outputs


def test_pack_encoder_splits_decoder_weights():
    """[up | skip] is the packed weight cut at the column where the stage's own features begin, both halves contiguous.  'bn': the packed
    weight is the Linear's times the BatchNorm's row scale gamma / sqrt(var + eps) - computed here from the state dict, not from the
    packed matrix -, so both halves carry it; the folded bias stays whole with the skip GEMM.  decoder2 has no norm: its halves are the
    Linear's own columns."""
    from cofii2p_amd import kpfpn
    from cofii2p_amd.spec import synth_state_dict

    for norm in ("gn", "bn", "ln"):
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth_state_dict(norm=norm).items()}
        P = kpfpn.pack_encoder(sd)
        for name, upc, cin, cout in DEC:
            p = "pc_encoder.%s." % name
            up, skip = P[p + "mlp.up.weight"], P[p + "mlp.skip.weight"]
            assert up.is_contiguous() and skip.is_contiguous()
            assert tuple(up.shape) == (cout, upc) and tuple(skip.shape) == (cout, cin - upc)
            assert torch.equal(torch.cat([up, skip], 1), P[p + "mlp.weight"])
            w, b = sd[p + "mlp.weight"].double(), sd[p + "mlp.bias"].double()
            if norm == "bn" and (p + "norm.running_mean") in sd:
                s_ = sd[p + "norm.weight"].double() / torch.sqrt(sd[p + "norm.running_var"].double() + 1e-5)
                assert float(s_.min()) != 1.0 or float(s_.max()) != 1.0   # the fold is not the identity on the synthetic weights
                b = b * s_ + sd[p + "norm.bias"].double() - sd[p + "norm.running_mean"].double() * s_
                w = w * s_[:, None]
            assert torch.equal(up, w[:, :upc].float()) and torch.equal(skip, w[:, upc:].float())
            assert torch.equal(P[p + "mlp.bias"], b.float())
