"""Records the bits of every engine entry point that runs a program, on ONE build, as tests/golden/engine_bits.npz;
tests/test_engine_bits_gpu.py replays the same calls on the current build and compares.

    python tests/golden/make_engine_bits.py            # needs a GPU; DD_LIB= / DD_LIB_F16= record another build of the libraries

Run it on the build whose engine is to be pinned (the commit BEFORE a change to how the engine builds, plans or runs its programs), never
to make a failing test pass.  The committed file was recorded at commit de4e83d, before engine_exec.cpp ran its ops through one function
per op kind and one gradient fan-out.

Engines (batch 2, each in the bf16 and in the fp16 library): 'tiny' (tiny_config with the VAE encoder and the text tower), 'tiny_sdxl' (both
text towers, VAE encoder, text_time conditioning), 'tiny_vit' and 'tiny_mbv2' (tiny_config with the ViT / the MobileNetV2 guide): the smallest
shapes that run every op kind and both reverse paths (bf16 and fp32 programs).  Outputs per engine: transform guidance over two chained
steps (z, score, dE/dz0), direct guidance (z, x0, score, dE/dz), a plain step (z, x0), unet_vjp, decode_vjp, guide_vjp, decode, vae_encode and
text_encode / text_encode_tower where the engine has the encoders, and one `expand` per guidance type.  Latents, scores and gradients are
stored as raw bits (uint8 views of the fp32 tensors), image-shaped outputs (IMAGES) as SHA-256, which keeps the file under the
repository's size limit.  Every engine is built and replayed twice and the file is not written unless the two replays agree."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "engine_bits.npz")
KINDS = ("tiny", "tiny_sdxl", "tiny_vit", "tiny_mbv2")
ENGINES = [(kind, act) for act in ("bf16", "fp16") for kind in KINDS]
N_STEPS, START, FIRST, COUNT = 10, 5, 6, 2
# image-shaped outputs [B,3,.,.]: the decoded images and guide_vjp's gradient with respect to the guide's input image
IMAGES = ("decode", "guide_vjp", "expand_none/image", "expand_transform/image", "expand_direct/image")


def make_engine(kind, act):
    import torch
    import torch.nn.functional as F
    from distdiff_amd.config import GuideConfig, tiny_config, tiny_sdxl_config
    from distdiff_amd.engine import Engine
    from distdiff_amd.scheduler import DDIMSchedule
    from distdiff_amd.weights import synthetic_weights
    import make_engine_plans as MP
    B = 2
    cfg = tiny_sdxl_config(max_batch=B) if kind == "tiny_sdxl" else tiny_config(max_batch=B)
    if kind in ("tiny_vit", "tiny_mbv2"):
        cfg.guide = GuideConfig(**(MP.VIT if kind == "tiny_vit" else MP.MBV2))
    encoders = kind in ("tiny", "tiny_sdxl")
    g = torch.Generator().manual_seed(31 + KINDS.index(kind))
    L, T, D, W = cfg.latent_size, cfg.text_len, cfg.guide.feature_dim, cfg.unet.cross_attention_dim
    S = cfg.guide.input_size
    fx = dict(z=torch.randn(B, 4, L, L, generator=g), lat=torch.randn(B, 4, L, L, generator=g) * 0.9, noise=torch.randn(B, 4, L, L, generator=g),
              e=torch.rand(B, 4, 1, 1, generator=g), b=torch.randn(B, 4, 1, 1, generator=g) * 0.3,
              emb=torch.randn(2 * B, T, W, generator=g), Pc=F.normalize(torch.randn(5, D, generator=g), dim=-1),
              Pg=F.normalize(torch.randn(5, 3, D, generator=g), dim=-1), targets=torch.tensor([1, 3]),
              g_eps2=torch.randn(2 * B, cfg.unet.out_channels, L, L, generator=g), g_image=torch.randn(B, 3, 8 * L, 8 * L, generator=g),
              images=torch.rand(B, 3, S, S, generator=g) * 2 - 1, g_feats=torch.randn(B, D, generator=g),
              pixels=torch.rand(B, 3, 8 * L, 8 * L, generator=g) * 2 - 1,
              ids=torch.randint(0, cfg.text.vocab_size, (2 * B, T), generator=g))
    eng = Engine(cfg, synthetic_weights(cfg, seed=0, num_classes=5, encoders=encoders), enable_grad=True, max_guidance_period=2, act_dtype=act)
    sched = DDIMSchedule(cfg.scheduler)
    ts = sched.set_timesteps(N_STEPS)
    eng.set_schedule(ts, sched.alphas_cumprod, sched.final_alpha_cumprod, guidance_period=2)
    eng.set_prototypes(fx["Pc"], fx["Pg"])
    eng.set_prompt(fx["emb"].cuda())
    if cfg.unet.add_time_dim:
        eng.set_added_cond(torch.randn(2 * B, cfg.unet.add_text_dim, generator=g),
                           torch.tensor([[128.0, 96.0, 0.0, 8.0, 128.0, 128.0], [64.0, 64.0, 4.0, 0.0, 128.0, 128.0]] * 2))
    eng.set_sample_weights([1.0, 1.0])
    return cfg, eng, fx, encoders


def outputs(cfg, eng, fx, encoders):
    """Every recorded output of one engine -> {name: tensor}."""
    o = {}
    o["transform/z"], o["transform/score"], o["transform/grad"] = eng.transform_guidance(fx["z"], fx["targets"], fx["e"], fx["b"], 5, 2)
    o["direct/z"], o["direct/x0"], o["direct/score"], o["direct/grad"] = eng.direct_guidance(fx["z"], fx["targets"], 7)
    o["step/z"], o["step/x0"] = eng.denoise_step(fx["z"], 8)
    o["unet_vjp"] = eng.unet_vjp(fx["z"], 3, fx["g_eps2"])
    o["decode_vjp"] = eng.decode_vjp(fx["lat"], fx["g_image"])
    o["guide_vjp"] = eng.guide_vjp(fx["images"], fx["g_feats"])
    o["decode"] = eng.decode(fx["lat"])
    if encoders:
        o["vae_encode/latents"], o["vae_encode/moments"] = eng.vae_encode(fx["pixels"], fx["noise"], return_moments=True)
        if cfg.text2 is None:
            o["text_encode"] = eng.text_encode(fx["ids"])
        else:
            o["text_tower0"] = eng.text_encode_tower(0, fx["ids"])
            o["text_tower1/hidden"], o["text_tower1/pooled"] = eng.text_encode_tower(1, fx["ids"], pooled=True)
    for name, gt in (("none", None), ("transform", "transform_guidance"), ("direct", "direct_guidance")):
        z, img, score = eng.expand(fx["lat"], fx["noise"], fx["e"], fx["b"], fx["targets"], START, gt, FIRST, COUNT)
        o["expand_%s/z" % name], o["expand_%s/image" % name], o["expand_%s/score" % name] = z, img, score
    return o


def replay(kind, act):
    """-> {"<act>/<kind>/<output>": uint8 array (the raw bits, or for an image the 32 bytes of its SHA-256)}."""
    import torch
    cfg, eng, fx, encoders = make_engine(kind, act)
    try:
        got = {}
        for name, t in outputs(cfg, eng, fx, encoders).items():
            torch.cuda.synchronize()
            assert torch.isfinite(t).all(), name
            raw = t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)
            got["%s/%s/%s" % (act, kind, name)] = np.frombuffer(hashlib.sha256(raw.tobytes()).digest(), np.uint8) if name in IMAGES else raw.copy()
        return got
    finally:
        eng.close()


def load():
    with np.load(PATH) as f:
        return {k: f[k] for k in f.files}


def main():
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    rec = {}
    for kind, act in ENGINES:
        first, second = replay(kind, act), replay(kind, act)
        unstable = [k for k in first if not np.array_equal(first[k], second[k])]
        if unstable:
            raise SystemExit("not written: outputs do not reproduce on this build: " + ", ".join(unstable))
        rec.update(first)
        print("%s/%s: %d outputs" % (act, kind, len(first)), flush=True)
    np.savez_compressed(PATH, **rec)
    from distdiff_amd import _lib
    print("wrote %s: %d outputs, %d bytes, libraries %s %s" % (PATH, len(rec), os.path.getsize(PATH), _lib.LIB_PATH, _lib.LIB_PATH_F16))


if __name__ == "__main__":
    main()
