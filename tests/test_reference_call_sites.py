"""Drop-in conformance by static analysis (no GPU needed).

The reference's CLIs cannot be executed against the facade on a GPU box (the product has no CPU path).  What CAN be checked is that
everything those scripts DO with the model is served by the facade: every keyword they pass to load_tokenhmr, every attribute they
touch on the returned model, every key they read from the output dict — collected from the reference's own sources with `ast` by
oracle/gen_golden_call_sites.py and frozen in tests/golden/reference_call_sites.json, compared here with what tokenhmr_amd.model
declares (its signature, its class, the dict literal of TokenHMR._pack).  The loop bodies themselves run on the GPU box in
tests/test_gpu_pipeline.py."""
import ast
import inspect
import json
import os

from conftest import GOLDEN_DIR

with open(os.path.join(GOLDEN_DIR, "reference_call_sites.json")) as _f:
    REF = json.load(_f)


def _facade_output_keys():
    from tokenhmr_amd import model as M
    tree = ast.parse(inspect.getsource(M))
    pack = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "_pack")
    keys, nested = set(), {}
    for n in ast.walk(pack):
        if isinstance(n, ast.Dict):
            for k, v in zip(n.keys, n.values):
                if isinstance(k, ast.Constant):
                    keys.add(k.value)
                    if isinstance(v, ast.Dict):
                        nested[k.value] = {kk.value for kk in v.keys if isinstance(kk, ast.Constant)}
    return keys, nested


def test_load_tokenhmr_accepts_every_keyword_the_reference_passes():
    from tokenhmr_amd.model import load_tokenhmr
    params = set(inspect.signature(load_tokenhmr).parameters)
    ref_sig = REF["load_tokenhmr_params"]
    assert ref_sig, "reference load_tokenhmr not found"
    assert set(ref_sig) <= params, (ref_sig, params)                       # same names (lib/models/__init__.py:3)
    assert list(inspect.signature(load_tokenhmr).parameters)[:len(ref_sig)] == ref_sig      # same positional order
    used = set()
    for c in REF["load_tokenhmr_calls"]:
        assert c["positional_args"] == 0, f"{c['script']}: positional call"          # the scripts call it by keyword
        used |= set(c["keywords"])
    assert {c["script"] for c in REF["load_tokenhmr_calls"]} == {"eval.py", "demo.py", "track.py"}
    assert used and used <= params, (used, params)


def test_every_model_attribute_the_scripts_touch_exists_on_the_facade():
    from tokenhmr_amd.model import TokenHMR
    init = ast.parse(inspect.getsource(TokenHMR))
    inst_attrs = {n.attr for n in ast.walk(init) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "self"}
    have = set(dir(TokenHMR)) | inst_attrs
    touched = set(REF["model_attrs"])
    # track.py wraps the model in a PHALP predictor class; what it calls on it is forward(batch) through __call__
    assert touched, "no model.<attr> use found in the reference scripts"
    missing = {a for a in touched if a not in have}
    assert not missing, f"the reference scripts use model.{missing}, the facade has no such attribute"
    # model.smpl.faces (demo.py:52)
    assert REF["demo_reads_model_smpl_faces"]
    from tokenhmr_amd.model import _SmplHandle
    assert "faces" in {n.attr for n in ast.walk(ast.parse(inspect.getsource(_SmplHandle))) if isinstance(n, ast.Attribute)}


def test_every_output_key_the_reference_reads_is_produced():
    keys, nested = _facade_output_keys()
    read = set(REF["output_keys_read"])            # demo.py / eval.py `out[...]`, track.py `model_out[...]`, Evaluator.__call__ `output[...]`
    assert {"pred_vertices", "pred_keypoints_3d", "pred_cam", "pred_cam_t"} <= read, read
    missing = read - keys
    assert not missing, f"the reference reads output keys {missing} that TokenHMR._pack does not produce"
    # the output dict of the reference's forward_step (tokenhmr.py:156-188): every key it sets at inference is produced too
    set_keys = set(REF["forward_step_output_keys"])
    assert set_keys, "no output[...] assignment found in forward_step"
    assert set_keys <= keys, (set_keys - keys)
    assert nested.get("pred_smpl_params") == {"global_orient", "body_pose", "betas"}


def test_tokenizer_dropins_keep_the_reference_constructors_and_call_sites():
    """tokenhmr_amd.tokenizer.DecodeTokens / EncodeTokens: the reference classes' constructor parameters come first, in order, with the same
    defaults (vanilla_pose_vqvae.py:258-262, :304-307), and the one place the reference instantiates and calls DecodeTokens
    (heads/token_classifier.py: Proxy) passes nothing the drop-in does not take."""
    from tokenhmr_amd import tokenizer as T
    for cls_name in ("DecodeTokens", "EncodeTokens"):
        ref = REF["tokenizer_classes"][cls_name]
        ref_args, ref_defaults = ref["init_params"], ref["init_defaults"]
        mine = inspect.signature(getattr(T, cls_name).__init__)
        names = list(mine.parameters)[1:]
        assert names[:len(ref_args)] == ref_args, (cls_name, names, ref_args)
        assert [mine.parameters[a].default for a in ref_args] == ref_defaults, cls_name
        assert ref["forward_params"] == 2 and len(inspect.signature(getattr(T, cls_name).forward).parameters) == 2      # (self, x)
    # the reference's own call site (token_classifier.py:85): eval('VanillaDecodeTokens')(tokenizer_checkpoint_path), handed to Proxy, which
    # moves it with .to(x.device) and calls it with the token probabilities (:12-20)
    calls = REF["token_classifier_eval_calls"]
    assert calls, "the reference no longer instantiates the tokenizer through eval(...)(ckpt_path) in token_classifier.py?"
    ok = set(inspect.signature(T.DecodeTokens.__init__).parameters)
    for c in calls:
        assert c["positional_args"] == 1 and all(k in ok for k in c["keywords"]), c
    used = set(REF["proxy_tokenizer_attrs"])
    assert used <= {"to"} and all(hasattr(T.DecodeTokens, a) for a in used | {"__call__"}), used
