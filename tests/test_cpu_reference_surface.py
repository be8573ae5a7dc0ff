"""The reference's own `model/blocks.py` and `model/transforms.py` load UNCHANGED against the MinkowskiEngine / compressai
surfaces of this build (north_star: "model/transforms.py and model/blocks.py load unchanged").  What they build on those
surfaces is pinned in tests/golden/reference_surface.json (tests/golden/make_reference_surface.py, data only): every surface
name they use, and per transform its module tree and state_dict.  The build's modules must match it key for key and accept
parameters of the reference's shapes."""
import importlib
import json
import os
import sys

import pytest
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_surface.json")


@pytest.fixture()
def reference_surface():
    import unified_point_cloud_compression_amd as upcc
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] in ("MinkowskiEngine", "compressai")}
    for k in saved:
        del sys.modules[k]
    upcc.install_shims(force=True)
    try:
        with open(FIXTURE) as f:
            yield json.load(f)
    finally:
        for k in list(sys.modules):
            if k.split(".")[0] in ("MinkowskiEngine", "compressai"):
                del sys.modules[k]
        sys.modules.update(saved)


def test_reference_transforms_construct_on_the_shim(reference_surface):
    ref = reference_surface
    from unified_point_cloud_compression_amd.model import transforms as mine
    from unified_point_cloud_compression_amd.model import blocks as my_blocks
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    assert importlib.import_module("MinkowskiEngine") is ME          # `import MinkowskiEngine as ME` in the reference files
    for name in ref["surface"]:                                     # every ME.* / compressai name they use resolves
        mod, attr = name.rsplit(".", 1)
        assert hasattr(importlib.import_module(mod), attr), name
    cfg = ref["config"]
    for cls, want in ref["transforms"].items():
        my = getattr(mine, cls)(cfg)
        sd_m = my.state_dict()
        assert list(sd_m) == [k for k, _ in want["state_dict"]], cls
        for k, shape in want["state_dict"]:
            assert list(sd_m[k].shape) == shape, (cls, k)
        mods = dict(my.named_modules())
        for name, qual in want["shim_modules"].items():               # the same shim layer at the same place
            assert f"{type(mods[name]).__module__}.{type(mods[name]).__name__}" == qual, (cls, name)
        for name in want["bias_free"]:
            assert mods[name].bias is None, (cls, name)
        g = torch.Generator().manual_seed(0)                        # the build's modules accept the reference's parameters
        my.load_state_dict({k: torch.rand(shape, generator=g) for k, shape in want["state_dict"]})
    gdn = ref["gdn_inverse_128"]
    g = my_blocks.MinkowskiGDN(128, inverse=True)
    assert g.inverse == gdn["inverse"] and list(g.gamma.shape) == gdn["gamma"] and g.kernel_size == gdn["kernel_size"]
    sd = dict(ref["transforms"]["SparseSynthesisTransform"]["state_dict"])
    assert sd["up_1.2.kernel"] == [125, 128, 128] and sd["color_conv.0.kernel"] == [32, 3]   # ME layout (A.4)
    assert sd["down_conv.kernel"] == [27, 1, 1]


def test_reference_loss_constructs_pooling_stubs(reference_surface):
    import unified_point_cloud_compression_amd.MinkowskiEngine as ME
    # loss.py:124-125,185 only construct these
    ME.MinkowskiAvgPooling(kernel_size=3, stride=1, dimension=3)
    ME.MinkowskiChannelwiseConvolution(1, kernel_size=3, stride=1, dimension=3)
