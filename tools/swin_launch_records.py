#!/usr/bin/env python
"""The Swin trunk's launch sequence as the profile records see it: one profiled forward per configuration below, each record
reduced to (kind, kernel, flops, bytes) — no timings.  The configurations reach every branch of swin_run (csrc/plan.hip):
fused and un-fused embedding, tails and merges, bias image and gather attention, padded partitions, fp16 and fp32 streams,
feature taps and the stage split.  tests/test_gpu_swin_launches.py re-runs them against the file.
    python tools/swin_launch_records.py            (writes tests/swin_launch_records.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "swin_launch_records.json")


def _trunk(cfg, dtype, wseed=0, hot_table=None):
    """A SwinTransformer3D of `cfg` on the builder's "stress" weights (the default init for Swin-B: its synthetic set takes
    long to draw and no record depends on the values); `hot_table`: one table given entries of +-40 (its block keeps the gather)."""
    import torch
    from kvq_amd import _abi
    from kvq_amd.models.backbones.swin_backbone import SwinTransformer3D
    torch.manual_seed(0)
    bb = SwinTransformer3D(embed_dim=cfg.embed_dim, depths=list(cfg.depths), num_heads=list(cfg.num_heads), window_size=cfg.window,
                           frag_biases=list(cfg.frag_biases), operand_dtype=dtype)
    if cfg.embed_dim == 96:
        from kvq_amd.utils import synth
        w = synth.synth_swin_weights(cfg, wseed, "stress")
        if hot_table:
            tab = w[hot_table].copy()
            tab[::97] = 40.0
            tab[5::193] = -40.0
            w[hot_table] = tab
        bb.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    bb.operand_dtype = _abi.dtype_code(dtype)
    bb.dense_bias = True
    return bb.to("cuda:0").eval()


def _fragments(B, T):
    """uint8 frames + sampler draws of a 7 x 7 grid of 32 x 32 fragments (a T x 224 x 224 clip read through the embedding launch)"""
    import torch
    from kvq_amd import kernels
    g = torch.Generator().manual_seed(77)
    Hs, Ws, dev = 300, 420, "cuda:0"
    vids = [torch.randint(0, 256, (3, T, Hs, Ws), dtype=torch.uint8, generator=g).to(dev) for _ in range(B)]
    gh = torch.tensor([min(Hs // 7 * i, Hs - 32) for i in range(7)]).view(7, 1, 1)
    gw = torch.tensor([min(Ws // 7 * i, Ws - 32) for i in range(7)]).view(1, 7, 1)
    hs = [(torch.randint(Hs // 7 - 32, (7, 7, T // 8), generator=g) + gh).int().to(dev) for _ in range(B)]
    ws = [(torch.randint(Ws // 7 - 32, (7, 7, T // 8), generator=g) + gw).int().to(dev) for _ in range(B)]
    return kernels.FragmentSource(vids, hs, ws, 7, 7, 32, 32, 8, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375))


def _clip(B, T, H, W):
    import torch
    from kvq_amd.utils import synth
    return torch.from_numpy(synth.synth_clip(5, T, H, W, batch=B)).to("cuda:0")


def _run(name):
    """(the trunk, B, (T, H, W), a function running the forward) of configuration `name`"""
    from kvq_amd.utils import synth
    T_ = synth.SWIN_T_GRPB
    if name.startswith("t_frag_"):                       # t_frag_<dtype>[_fp32stream]: the bench's step, sampler inside the embedding
        dtype = name.split("_")[2]
        bb = _trunk(T_, dtype)
        bb.residual16 = not name.endswith("_fp32stream")
        x = _fragments(1, 32)
        return bb, 1, (32, 224, 224), lambda: bb({"technical": x})
    if name == "t_unfused_16x64":                        # im2col / GEMM / LayerNorm launches, proj / fc1 / fc2 chain, gather attention
        bb = _trunk(T_, "fp16")
        bb.fused_tail = bb.dense_bias = False
        x = _clip(1, 16, 64, 64)
        return bb, 1, (16, 64, 64), lambda: bb({"technical": x})
    if name == "t_gather_block_8x64":                    # block 2's bias table past +-16: that block alone takes the gather path
        bb = _trunk(T_, "fp16", 11, "layers.1.blocks.0.attn.relative_position_bias_table")
        x = _clip(1, 8, 64, 64)
        return bb, 1, (8, 64, 64), lambda: bb({"technical": x})
    if name == "t_taps_32x224":                          # feature taps: fp32 stream in every stage
        bb = _trunk(T_, "fp16")
        x = _clip(1, 32, 224, 224)
        return bb, 1, (32, 224, 224), lambda: bb({"technical": x}, multi=True)
    if name == "t_stages_32x224":                        # KSVQE's stage split: stages 0-1, 2, 3
        bb = _trunk(T_, "fp16")
        x = _clip(1, 32, 224, 224)

        def split():
            s1 = bb.forward_stages(x, 0, 1)
            s2 = bb.forward_stages(s1, 2, 2, geometry=(32, 224, 224))
            return bb.forward_stages(s2, 3, 3, geometry=(32, 224, 224), want_feat=True)
        return bb, 1, (32, 224, 224), split
    if name == "b_fp16_64x256":                          # Swin-B: padded partitions, un-fused merges writing fp16
        bb = _trunk(synth.SWIN_B_GRPB, "fp16")
        x = _clip(1, 64, 256, 256)
        return bb, 1, (64, 256, 256), lambda: bb({"technical": x})
    raise KeyError(name)


CONFIGS = ["t_frag_fp16", "t_frag_bf16", "t_frag_fp16_fp32stream", "t_frag_bf16_fp32stream", "t_unfused_16x64", "t_gather_block_8x64",
           "t_taps_32x224", "t_stages_32x224", "b_fp16_64x256"]


def records(name):
    """[kind, kernel, flops, bytes] of every profile record of one forward of configuration `name`"""
    import torch
    bb, B, (T, H, W), fwd = _run(name)
    dev = torch.device("cuda:0")
    with torch.no_grad():
        fwd()                                            # plan, packed weights and bias images first: the profiled forward is a steady one
        bb.profile(B, T, H, W, dev, True)
        fwd()
        torch.cuda.synchronize()
        recs = bb.profile_read(B, T, H, W, dev)
        bb.profile(B, T, H, W, dev, False)
    return [[r["kind"], r["kernel"], r["flops"], r["bytes"]] for r in recs]


def main():
    import kvq_amd  # noqa: F401
    out = {name: records(name) for name in CONFIGS}
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: [\n" + ",\n".join(json.dumps(r) for r in v) + "\n]" for k, v in out.items()) + "\n}\n")
    print(OUT, {k: len(v) for k, v in out.items()}, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
