"""pdengine: MI355X-native Prompt-Diffusion DDIM sampling engine (host side).

The compute path is ``csrc/libpdengine.so`` (hand-written gfx950 HIP kernels behind
the C ABI of ``include/pdengine.h``); this package is the Python host that mirrors
the reference's ``PromptDiffusionPipeline.__call__`` (pipeline_prompt_diffusion.py:890)
and ``DDIMSampler.sample`` (cldm/ddim_hacked.py:55) surfaces over ctypes.
"""
__version__ = "0.1.0"

_PIPELINES = ("PromptDiffusionPipeline", "PromptDiffusionImg2ImgPipeline", "PromptDiffusionInpaintPipeline")
_SD3_PIPELINES = ("StableDiffusion3PromptDiffusionPipeline", "StableDiffusion3PromptDiffusionImg2ImgPipeline",
                  "StableDiffusion3PromptDiffusionInpaintPipeline")


def __getattr__(name):   # the pipelines and the annotators, imported on first use (the package itself stays light)
    if name in _PIPELINES:
        from . import pipeline
        return getattr(pipeline, name)
    if name in _SD3_PIPELINES:
        from . import pipeline_sd3
        return getattr(pipeline_sd3, name)
    if name in ("HEDdetector", "CannyDetector", "MLSDdetector"):   # the annotators (annotators.py), NumPy only on import
        from . import annotators
        return getattr(annotators, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
