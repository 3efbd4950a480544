"""Golden data for tests/test_reference_dropin.py from the upstream reference (build container only, like make_golden.py):
the release config train_medium.yaml's MODEL.HEAD and DATA_PRESET nodes, and the checkpoint surface of the reference's own
POEM_Generalized_Head built from them -- every state_dict key (live and dead tensors) with its shape and dtype, in order,
plus the head attributes the drop-in test compares.  No tensor values: the test fills the surface with seeded values.

  python tests/golden/make_golden_dropin.py        ->  tests/golden/dropin.json"""
import json
import os
import sys

GOLDEN = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [GOLDEN]
sys.dont_write_bytecode = True


def main():
    import ref_harness as rh
    CN, ref_build_head = rh.setup()
    import lib.models.heads.ptEmb_head as ref_head_mod
    cfg, y = rh.load_head_cfg(CN, "medium")
    ref = ref_build_head(cfg, data_preset=CN(y["DATA_PRESET"]))
    assert type(ref) is ref_head_mod.POEM_Generalized_Head
    sd = ref.state_dict()
    out = {"source": "config/release/train_medium.yaml + lib/models/heads/ptEmb_head.py POEM_Generalized_Head (upstream)",
           "head_cfg": y["MODEL"]["HEAD"], "data_preset": y["DATA_PRESET"],
           "num_preds": int(ref.num_preds), "nsample": int(ref.nsample),
           "state_dict": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()]}
    with open(os.path.join(GOLDEN, "dropin.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(f"dropin.json: {len(sd)} state_dict entries")


if __name__ == "__main__":
    main()
