"""What tests/golden/prepared_weights.json pins: the kernel-ready tensors every model mirror prepares from its parameters and
buffers (operand cast with the fp16 clamp, BatchNorm fold, K padding, stem spreading, packed stem images), as one sha256 per
tensor over (dtype, shape, raw bytes).  Pure torch on the CPU.  Shared by tests/golden/make_prepared_golden.py (which wrote the
file from the code BEFORE the preparation moved into ``_prepared.py``) and tests/test_prepared_weights_cpu.py (which asserts
every digest against the present code).

Inputs are integer arithmetic on ``torch.arange`` divided by powers of two: no random generator, no transcendental function, so
the bits are the same on any (little-endian) host.  Running variances are odd/8 (positive, never 1), running means odd/16
(never 0), every 1-D ``weight`` (the BatchNorm / LayerNorm gains) odd/8 (never 1); row 1 of every matrix / conv weight is
scaled by 2^24 so that the folded row passes 65504 in magnitude: fp16 must clamp there, bf16 must not."""
import hashlib

import torch

DTYPES = ("fp16", "bf16")


def fill(module):
    """Overwrite every parameter and buffer of ``module`` in place with its deterministic pattern."""
    with torch.no_grad():
        for i, (name, t) in enumerate(list(module.named_parameters()) + list(module.named_buffers())):
            k = torch.arange(t.numel(), dtype=torch.int64).reshape(t.shape)
            leaf = name.rsplit(".", 1)[-1]
            if not t.is_floating_point():
                t.copy_((k + i) % 5)                                    # num_batches_tracked
            elif leaf == "running_var":
                t.copy_((2 * ((k + i) % 11) + 1).to(torch.float32) / 8)
            elif leaf == "running_mean":
                t.copy_((2 * ((k + i) % 9) - 9).to(torch.float32) / 16)
            elif leaf == "weight" and t.dim() == 1:
                t.copy_((2 * ((k + i) % 7) + 1).to(torch.float32) / 8)
            else:
                t.copy_(((k * 37 + 11 * i) % 101 - 50).to(torch.float32) / 64)
                if t.dim() >= 2 and t.shape[0] >= 2:
                    t[1] *= 2.0 ** 24


def digest(t):
    if not torch.is_tensor(t):
        return hashlib.sha256(repr(t).encode()).hexdigest()
    t = t.detach().cpu().contiguous()
    head = f"{t.dtype}|{tuple(t.shape)}|".encode()
    return hashlib.sha256(head + t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def flatten(obj, prefix, out):
    """Nested dict / list / tuple of tensors -> out[prefix/key/index...] = digest; non-tensor leaves (kernel / stride / pad tuples
    of ints, Python floats) are digested through their repr."""
    if isinstance(obj, dict):
        for k, v in obj.items():
            flatten(v, f"{prefix}/{k}", out)
    elif isinstance(obj, (list, tuple)) and any(torch.is_tensor(v) or isinstance(v, (dict, list, tuple)) for v in obj):
        for i, v in enumerate(obj):
            flatten(v, f"{prefix}/{i}", out)
    else:
        out[prefix] = digest(obj)
    return out


def _slow_stem8_loop(wt, taps, cin):
    """The slow stem's (taps, 3)-ordered columns spread to (taps, 8), K padded to 32: written out element by element."""
    kpad = -(-taps * 8 // 32) * 32
    t8 = torch.zeros(wt.shape[0], kpad, dtype=wt.dtype)
    for tap in range(taps):
        for c in range(cin):
            t8[:, tap * 8 + c] = wt[:, tap * cin + c]
    return t8


def collect():
    """{``model/dtype/tensor-key``: sha256} of every prepared tensor, for fp16 and bf16 operands."""
    import kvq_amd  # noqa: F401
    from kvq_amd import _abi, kernels
    from kvq_amd.models.backbones import KSVQE_model, clip_visual, ksvqe_modules as KM, simpleVQA_model, slowfast_model
    from kvq_amd.models.head import VQAHead

    out = {}
    resnet = simpleVQA_model.ResNet(layers=(2, 1, 1, 1))
    tv50 = KM.get_network("resnet50")
    sf = slowfast_model.slowfast()
    clip = clip_visual.CLIP_extractor_addadapter_cls(layers=2)
    contrique = KM.CONTRIQUE_model(KM.get_network("resnet50"), 2048)
    ksvqe = KSVQE_model.KSVQE()
    cross = KM.crossattention1(768, 12)
    head = VQAHead()
    adapters = [ksvqe.dist_adapter] + list(ksvqe.semantic_adapter) + list(ksvqe.distortion_adapter)
    names = ["dist_adapter"] + [f"semantic_adapter.{i}" for i in range(len(ksvqe.semantic_adapter))] + \
            [f"distortion_adapter.{i}" for i in range(len(ksvqe.distortion_adapter))]
    for m in [resnet, tv50, sf, clip, contrique.projector, cross, head] + adapters:
        fill(m)
    stem_key = "feature_extraction.0.multipathway_blocks.0"
    for dt in DTYPES:
        code = _abi.dtype_code(dt)
        for m in (resnet, tv50, sf, clip, contrique, ksvqe, cross):
            m.operand_dtype = code
        flatten(resnet._weights("cpu"), f"ResNet/{dt}", out)
        flatten(tv50._weights("cpu"), f"TorchvisionResNet50/{dt}", out)
        Wt = dict(sf._weights("cpu"))
        wt = Wt[stem_key][0]
        # the 8-channel slow-stem weight and the packed 1x7x7 stem image (what the one-call plan streams)
        Wt.setdefault(stem_key + "/stem8", _slow_stem8_loop(wt, 49, 3))
        Wt[stem_key + "/stem64"] = kernels.stem64_pack_weight(wt, wt.dtype)
        flatten(Wt, f"slowfast/{dt}", out)
        flatten(clip._weights("cpu"), f"CLIP/{dt}", out)
        p = contrique.projector
        flatten({"fold0": contrique._fold(p[0], p[1], "cpu"), "fold1": contrique._fold(p[3], p[4], "cpu")}, f"CONTRIQUE/{dt}", out)
        ad = ksvqe._adapters("cpu")
        flatten({n: ad[id(m)] for n, m in zip(names, adapters)}, f"KSVQE/{dt}", out)
        flatten({n: cross._w16(getattr(cross, n).weight, "cpu") for n in ("fc_q", "fc_k", "fc_v")}, f"crossattention1/{dt}", out)
        flatten(list(head._prepared("cpu")), f"VQAHead/{dt}", out)          # fp32 whatever the operand type: the same digests twice
    return out
