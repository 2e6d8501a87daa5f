"""Run by tests/test_stage_oracle_gpu.py in a child process with VSD_POISON=1, beside tests/poison_check.py: the program with every
per-frame switch on (per-frame prompts with a mix, per-frame options, seeded noise, Canny edges, colour match, keep masks) while every
buffer the engine allocates "uninitialised" starts as 0xFF bytes.  Prints one JSON line: per size, per frame, what
`stage_oracle.figures` compares with the stage oracle (r0, r1, r1 over the mixed latent pixels, mean LSB and PSNR over the restyled
pixels, whether the post stages are exact); the parent holds them to the bounds of the unpoisoned run."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    import stage_oracle as SO
    from oracle.pipeline import OraclePipeline
    from videosd_amd import blocks as BK
    from videosd_amd import config as C
    from videosd_amd import ops as O
    from videosd_amd import weights as W
    from videosd_amd.engine import Engine

    assert O.POISON or os.environ.get("VSD_POISON_CHECK_ANYWAY"), "run with VSD_POISON=1"
    wu = W.synthesize(W.unet_spec(C.MINI_UNET), "unet.", device="cuda")
    wc = W.synthesize(W.controlnet_spec(C.MINI_CONTROLNET), "cn.", device="cuda")
    wv = W.synthesize(W.taesd_spec(C.TAESD), "vae.", device="cuda")
    cpu = lambda w: {k: v.float().cpu() for k, v in w.items()}  # noqa: E731
    orc = OraclePipeline(C.MINI_UNET, C.MINI_CONTROLNET, cpu(wu), cpu(wc), cpu(wv))
    text_ab = SO.texts(C.MINI_UNET.cross_dim)
    out = {}
    for H, Wd in SO.SIZES:
        eng = Engine(O.HipOps(0), C.MINI_UNET, C.MINI_CONTROLNET, C.TAESD, wu, wc, wv)
        eng.set_text_embeds(text_ab[0])
        a, b = eng.build_prompt(text_ab[0]), eng.build_prompt(text_ab[1])
        SO.prepare_case(eng, "all", H, Wd, (a, b, BK.PromptMix([a, b], SO.MIX_WEIGHTS)), autotune=False)
        camera, masks = SO.frames(H, Wd), SO.masks(H, Wd)
        got = SO.launch_case(eng, "all", camera)
        before, eager = SO.frames_ahead_of_the_post_stages(eng, H, Wd)
        rows = []
        for f in range(SO.B):
            right = SO.oracle_case(orc, "all", H, Wd, f, text_ab, camera)
            fig = SO.figures(eng, f, right, camera[f], before[f], got[f], masks[f], SO.CASES["all"]["color_match"])
            fig["post_exact"] = bool(fig["post_exact"] and (eager[f] == got[f]).all())
            rows.append({k: (v if isinstance(v, bool) else round(float(v), 6)) for k, v in fig.items()})
        out[f"{Wd}x{H}"] = rows
        del eng
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
