"""tests/golden/checkpoint_layout.json: the state_dict layout of the REFERENCE model that
tests/test_checkpoint_reference.py exchanges checkpoints with (BeaUTyDETR, num_queries=64, butd=True, its text encoder
replaced by tests/model_fixtures.small_roberta(1) and frozen, as the test does), imported through tools/ref_import.py
(needs the reference checkout; the test itself does not).  One record per state_dict entry, in the reference's order:
    [name, shape, dtype, "param" | "buffer", requires_grad]
Only names, shapes and flags are stored: the test rebuilds a module with exactly this layout and fills it with the same
deterministic values (model_fixtures.fill_det_state) the reference model was given.
    python tools/gen_golden_checkpoint_layout.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import model_fixtures as MF  # noqa: E402
import ref_import  # noqa: E402


def main():
    mods = ref_import.load()
    ref = ref_import.build_reference_model(mods, seed=0, num_queries=64, butd=True)
    ref.text_encoder = MF.small_roberta(1)
    for p in ref.text_encoder.parameters():
        p.requires_grad = False
    params = dict(ref.named_parameters())
    buffers = dict(ref.named_buffers())
    records = []
    for name, v in ref.state_dict().items():
        if name in params:
            records.append([name, list(v.shape), str(v.dtype).replace("torch.", ""), "param", params[name].requires_grad])
        else:
            assert name in buffers, name
            records.append([name, list(v.shape), str(v.dtype).replace("torch.", ""), "buffer", False])
    # no shared parameters: named_parameters() is the state_dict's parameter entries in the same order
    assert list(params) == [r[0] for r in records if r[3] == "param"]
    out = os.path.join(ROOT, "tests", "golden", "checkpoint_layout.json")
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in records) + "\n]\n")
    print("wrote", out, len(records), "entries,", sum(r[3] == "param" for r in records), "parameters")


if __name__ == "__main__":
    main()
