"""TEST INFRASTRUCTURE ONLY — what the reference's scripts DO with the model, collected from its sources with `ast` and frozen as
tests/golden/reference_call_sites.json (names and literal defaults only): the keywords eval.py / demo.py / track.py pass to
load_tokenhmr and the reference's own signature of it, every `model.<attr>` they touch, every output key they (and the Evaluator) read,
the keys forward_step sets, the tokenizer classes' constructor parameters / defaults and their one call site in token_classifier.py.
tests/test_reference_call_sites.py checks the facade against the file.  Run with a checkout of the reference:
    python oracle/gen_golden_call_sites.py <reference checkout>      (or TOKENHMR_REFERENCE=<reference checkout>)"""
import ast
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = None            # <reference checkout>/tokenhmr, set in __main__
OUT = os.path.join(ROOT, "tests", "golden", "reference_call_sites.json")
SCRIPTS = ("eval.py", "demo.py", "track.py")


def _parse(rel):
    with open(os.path.join(REF, rel)) as f:
        return ast.parse(f.read())


def _subscript_keys(tree, names):
    """string keys k of `name[k]` loads for name in names"""
    keys = set()
    for n in ast.walk(tree):
        if isinstance(n, ast.Subscript) and isinstance(n.value, ast.Name) and n.value.id in names:
            s = n.slice
            if isinstance(s, ast.Constant) and isinstance(s.value, str):
                keys.add(s.value)
    return keys


def _attrs(tree, name):
    return {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == name}


def collect():
    res = {}
    # load_tokenhmr: the reference's positional parameters (lib/models/__init__.py:3) and how the scripts call it
    res["load_tokenhmr_params"] = next([a.arg for a in n.args.args] for n in ast.walk(_parse("lib/models/__init__.py"))
                                       if isinstance(n, ast.FunctionDef) and n.name == "load_tokenhmr")
    calls = []
    for script in SCRIPTS:
        for n in ast.walk(_parse(script)):
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == "load_tokenhmr":
                calls.append({"script": script, "positional_args": len(n.args), "keywords": sorted(k.arg for k in n.keywords)})
    res["load_tokenhmr_calls"] = calls
    # model.<attr> in the scripts; model.smpl.faces (demo.py:52)
    res["model_attrs"] = sorted(set().union(*(_attrs(_parse(s), "model") for s in SCRIPTS)))
    res["demo_reads_model_smpl_faces"] = any(isinstance(n, ast.Attribute) and n.attr == "faces" and isinstance(n.value, ast.Attribute)
                                             and n.value.attr == "smpl" for n in ast.walk(_parse("demo.py")))
    # output keys read by the scripts and by Evaluator.__call__(output, batch)
    read = _subscript_keys(_parse("demo.py"), {"out"}) | _subscript_keys(_parse("eval.py"), {"out"})
    read |= _subscript_keys(_parse("track.py"), {"model_out"}) | _subscript_keys(_parse("lib/utils/pose_utils.py"), {"output"})
    res["output_keys_read"] = sorted(read)
    # output[...] assignments of forward_step (tokenhmr.py:156-188)
    fs = next(n for n in ast.walk(_parse("lib/models/tokenhmr.py")) if isinstance(n, ast.FunctionDef) and n.name == "forward_step")
    set_keys = set()
    for n in ast.walk(fs):
        if isinstance(n, ast.Assign):
            for t in n.targets:
                if isinstance(t, ast.Subscript) and isinstance(t.value, ast.Name) and t.value.id == "output" and isinstance(t.slice, ast.Constant):
                    set_keys.add(t.slice.value)
    res["forward_step_output_keys"] = sorted(set_keys)
    # tokenizer classes (vanilla_pose_vqvae.py:258-262, :304-307): constructor parameters after self, their literal defaults, forward arity
    with open(os.path.join(os.path.dirname(REF), "tokenization", "models", "vanilla_pose_vqvae.py")) as f:
        tree = ast.parse(f.read())
    res["tokenizer_classes"] = {}
    for cls_name in ("DecodeTokens", "EncodeTokens"):
        cls = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == cls_name)
        init = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__init__")
        fwd = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "forward")
        res["tokenizer_classes"][cls_name] = {"init_params": [a.arg for a in init.args.args][1:],
                                              "init_defaults": [ast.literal_eval(d) for d in init.args.defaults],
                                              "forward_params": len(fwd.args.args)}
    # the reference's call site (token_classifier.py:85): eval('VanillaDecodeTokens')(tokenizer_checkpoint_path), and what Proxy does with it
    tc = _parse("lib/models/heads/token_classifier.py")
    res["token_classifier_eval_calls"] = [{"positional_args": len(n.args), "keywords": sorted(k.arg for k in n.keywords)} for n in ast.walk(tc)
                                          if isinstance(n, ast.Call) and isinstance(n.func, ast.Call) and isinstance(n.func.func, ast.Name)
                                          and n.func.func.id == "eval"]
    proxy = next(n for n in ast.walk(tc) if isinstance(n, ast.ClassDef) and n.name == "Proxy")
    res["proxy_tokenizer_attrs"] = sorted({n.attr for n in ast.walk(proxy) if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Attribute)
                                           and n.value.attr == "tokenizer"})
    return res


if __name__ == "__main__":
    top = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TOKENHMR_REFERENCE")
    if not top:
        sys.exit("usage: python oracle/gen_golden_call_sites.py <reference checkout>")
    REF = os.path.join(top, "tokenhmr")
    with open(OUT, "w") as f:
        json.dump(collect(), f, indent=1)
        f.write("\n")
    print("wrote", OUT)
