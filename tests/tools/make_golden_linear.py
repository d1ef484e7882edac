"""Generate the linear-attention fixtures by RUNNING THE REFERENCE (development container only).

    python tests/tools/make_golden_linear.py [--only micro|tiny]

In the style of make_golden.py (whose helpers it uses): the reference is imported through tests/tools/ref_shims.py and run on the CPU.
  linear_attention_micro.npz   `LinearAttention()` on the q / k / v of micro_ops.npz ((L, S) = (48, 80)), and
                               `LoFTREncoderLayer(128, 4, 'linear')` with the seeded weights and inputs of micro_ops.npz
  frame_tiny_linear.npz        the tiny frame in 'val' and 'test' mode through the reference model whose transformer is
                               `LocalFeatureTransformer(128, 4, ['self', 'cross'] * 4, 'linear')` (same 430 tensors: the attention
                               module has no parameters); the arrays of frame_tiny.npz, the 'test' mode ones in
  frame_tiny_linear_test.npz   (two files: each stays under the 1 MiB limit of a committed file - see gen_tiny)
The fixtures are data: expected outputs of the reference, nothing else.
"""
import argparse
import importlib
import os

import numpy as np
import torch

import make_golden as MG  # noqa: E402  (sets sys.path, imports ref_shims)


def gen_micro():
    MG.ref_shims.import_reference()
    tr = importlib.import_module("model.transformer.transformer")
    la = importlib.import_module("model.transformer.linear_attention")
    micro = np.load(os.path.join(MG.GOLD, "micro_ops.npz"))
    t = lambda name: torch.from_numpy(micro[name])
    out = {}
    with torch.no_grad():
        q, k, v = t("att_q")[None], t("att_k")[None], t("att_v")[None]
        out["lin_out"] = la.LinearAttention()(q, k, v)[0].reshape(q.shape[1], -1)
        lay = tr.LoFTREncoderLayer(128, 4, "linear")
        lay.load_state_dict({n[len("lay_w_"):]: t(n) for n in micro.files if n.startswith("lay_w_")}, strict=True)
        out["lay_out"] = lay(t("lay_x")[None], t("lay_src")[None])[0]
    np.savez_compressed(os.path.join(MG.GOLD, "linear_attention_micro.npz"), **{k_: v_.numpy() for k_, v_ in out.items()})
    print("linear_attention_micro.npz:", {k_: tuple(v_.shape) for k_, v_ in out.items()})


def build_linear_model():
    net = MG.ref_shims.import_reference()
    tr = importlib.import_module("model.transformer.transformer")
    sd = {k: torch.from_numpy(v) for k, v in MG.synth_state_dict().items()}
    model = net.CoFiI2P(MG.ref_shims.reference_options())
    model.transformer = tr.LocalFeatureTransformer(128, 4, ["self", "cross"] * 4, "linear")
    model.load_state_dict(sd, strict=True)
    assert list(model.state_dict().keys()) == list(sd.keys())
    model.eval()
    return model


def gen_tiny():
    """The arrays of frame_tiny.npz, kept under the size limit of a committed file: 'val' outputs, inputs' hashes and the transformer
    taps in frame_tiny_linear.npz, 'test' outputs in frame_tiny_linear_test.npz.  The taps of the encoders and up-samplers do not depend
    on the attention kind: they are checked here to equal those of frame_tiny.npz bit for bit and not stored a second time."""
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "frame.npz")   # (absolute: run_frame's join with the golden directory keeps it)
        MG.run_frame(build_linear_model(), path, frame_id=1, num_points=2048, pyr_seed=11, modes=("val", "test"))
        rec = dict(np.load(path))
    base = np.load(os.path.join(MG.GOLD, "frame_tiny.npz"))
    assert sorted(rec) == sorted(base.files)
    test, val = {}, {}
    for k, v in rec.items():
        if k.startswith("tap_") and not k.startswith("tap_transformer"):
            assert np.array_equal(v, base[k]), k
        elif k.startswith("test_"):
            test[k] = v
        else:
            val[k] = v
            if not (k.startswith("val_") or k.startswith("tap_")):
                assert np.array_equal(v, base[k]), k   # same seeds, same inputs
    np.savez_compressed(os.path.join(MG.GOLD, "frame_tiny_linear.npz"), **val)
    np.savez_compressed(os.path.join(MG.GOLD, "frame_tiny_linear_test.npz"), **test)
    print("frame_tiny_linear.npz:", sorted(val), "\nframe_tiny_linear_test.npz:", sorted(test))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    if args.only in (None, "micro"):
        gen_micro()
    if args.only in (None, "tiny"):
        gen_tiny()


if __name__ == "__main__":
    main()
