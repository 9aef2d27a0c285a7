"""Launch plans that tests compare against recorded ones (no GPU): the generators whose plans tests/golden/plans_r08.json
holds, and the normal form of a plan_summary that such recordings keep."""
import re

# name -> (model, configuration): between them every kind of fused-convolution step the planner makes
CASES = {
    # narrow launches only; mode 0 has the column-only fused upsample
    "gen_resnet_up0": ("gen_resnet", dict(tile_low=16, up_res=4, channels=4, upsampling_mode=0)),
    "gen_resnet_up2": ("gen_resnet", dict(tile_low=16, up_res=4, channels=4, upsampling_mode=2)),
    # two wide layers of two windows each
    "growing_wide": ("growing_gen", dict(tile_low=8, up_res=8, channels=4, first_gen=True, filter_size=3, use_res_net=True,
                                         first_nn_arch=False, start_fms=512, max_fms=256, add_adj=True)),
    # depth-to-space steps of 4 and 2 launches next to wide and narrow ones
    "growing_pixel_shuffle": ("growing_gen", dict(tile_low=8, up_res=8, channels=4, first_gen=True, filter_size=3,
                                                  use_res_net=True, first_nn_arch=False, start_fms=512, max_fms=512,
                                                  pixel_shuffle=True, add_adj=True)),
    # resBlock 0 is one conv2d_small_pair launch (test_abi_and_graph.py::test_fusion_plan)
    "gen_resnet_small_pair": ("gen_resnet", dict(tile_low=8, up_res=4, channels=1, upsampling_mode=2)),
}


def generator(case, prec, params=None, device="cuda:0"):
    from mpgan_amd import multipass as MP
    model, cfg = CASES[case]
    return MP.Generator(model, dict(cfg), params, prec, device=device)


def norm(plan):
    """every field of a plan_summary but the node ids and names, which count the graphs built before"""
    out = []
    for e in plan:
        d = {k: v for k, v in e.items() if k not in ("node", "post_add", "post_add_id", "segments")}
        d["op"] = re.sub(r"_\d+$", "", e["node"])
        d["has_post_add"] = e.get("post_add") is not None
        d["segments"] = [{k: (list(v) if isinstance(v, tuple) else v) for k, v in s.items() if k not in ("src", "src_id")}
                         for s in e.get("segments", [])]
        out.append(d)
    return out
