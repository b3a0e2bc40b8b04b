"""Guided decoding on the CPU: the regex -> byte DFA compiler against ``re``, the token table
against a per-token byte walk, JSON schemas, the engine (sync / async, mixed batches,
preemption, a small arena), the HTTP server and the CR."""
import asyncio
import itertools
import json
import random
import re
from dataclasses import replace

import numpy as np
import pytest
import torch

from mlopamd.models import build_model
from mlopamd.models.config import TINY_LLAMA
from mlopamd.runtime import guided as G
from mlopamd.runtime.backends import ByteTokenizer, HFTokenizer, LLMBackend
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import SamplingParams

# (pattern, the 6 symbols its strings are drawn from): every supported construct
PATTERNS = [
    (r"abc", "abcd x"), (r"a|b|cd", "abcd |"), (r"a*b+c?", "abc d*"), (r"(ab)*c", "abc()x"),
    (r"(?:a|b){2}", "ab{2}c"), (r"a{2,}", "a{2,}"), (r"a{1,3}b", "ab{1,3"), (r"[abc]+", "abcd[]"),
    (r"[^ab]c", "abc^\nd"), (r"[a-c0-1]*", "abc01d"), (r"\d+\.\d", "01.a\\d"), (r"\w\s\w", "a_ \t-1"),
    (r".b", "ab\n.x "), (r"a.*b", "ab\nxy."), (r"\n\t\\", "\n\t\\ant"), (r"\x41\x2e", "A.Bx41"),
    (r"\(\)\[\]", "()[]\\a"), (r"[\]\-a]+", "]-a\\b["), (r"[]a]b", "]ab[\\c"), (r"(a|b)*abb", "ab()|*"),
    (r"((a|b)c?){0,2}", "abc{}0"), (r"a?b?c?", "abc?d "), (r"x{0}y", "xy{0}a"), (r"[\d\s]x", "0 x\\ds"),
    (r"a{b", "a{b}c1"), (r"(|a)b", "ab|()c"), (r"[a\-z]", "a-zbm\\"), (r"[^\n]", "a\nb^\\n"),
    (r"\{\}\|\*\+\?", "{}|*+?"), (r"[é0-9]+é", "é09a1-"),
]


@pytest.mark.parametrize("pattern,alphabet", PATTERNS)
def test_regex_matches_re_fullmatch(pattern, alphabet):
    dfa, rx = G.regex_to_dfa(pattern), re.compile(pattern)
    for n in range(6):
        for tup in itertools.product(alphabet, repeat=n):
            s = "".join(tup)
            assert dfa.matches(s) == (rx.fullmatch(s) is not None), (pattern, s)


def test_regex_non_ascii():
    for pattern, s in [("é+", "éé"), (".", "é"), (".", "日"), ("[^a]", "😀"), ("[éa]b", "éb"), ("日本", "日本"),
                       ("a.c", "a€c"), ("[^a]", "a"), (".", "\n"), ("é", "e"), ("[éa]", "ü")]:
        assert G.regex_to_dfa(pattern).matches(s) == (re.fullmatch(pattern, s) is not None), (pattern, s)
    any_char = G.regex_to_dfa(".")
    # only well-formed UTF-8: no lone lead / continuation byte, overlong form or surrogate
    for bad in (b"\xc3", b"\x80", b"\xc0\xaf", b"\xe0\x80\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80"):
        assert not any_char.matches(bad), bad
    assert any_char.matches("\U0010ffff") and any_char.matches("ࠀ") and any_char.matches("퟿")


@pytest.mark.parametrize("pattern,names", [
    (r"(a)\1", "backreference"), (r"(?=a)b", "look-around"), (r"(?!a)b", "look-around"),
    (r"(?<=a)b", "look-around"), (r"(?<!a)b", "look-around"), (r"a*?", "lazy"), (r"a+?", "lazy"),
    (r"a??", "lazy"), (r"a{1,2}?", "lazy"), (r"a*+", "possessive"), (r"a++", "possessive"), (r"^a", "anchor"),
    (r"a$", "anchor"), (r"\bfoo", "anchor"), (r"\Aa", "anchor"), (r"[[:alpha:]]", "named character class"),
    (r"(?P<n>a)", "named group"), (r"(?i)a", "group extension"), (r"[é-ü]", "range"), (r"[^é]", "negated"),
    (r"\D", "escape"), (r"\pL", "escape"), (r"*a", "nothing to repeat"), (r"(a", "unbalanced"), (r"a)", "unbalanced"),
    (r"[a", "unterminated"), (r"a{2000}", "bound"), (r"a{3,1}", "max < min"), ("a\\", "backslash"),
])
def test_regex_unsupported_constructs_raise(pattern, names):
    with pytest.raises(ValueError, match=names):
        G.regex_to_dfa(pattern)


# ------------------------------------------------------------------ token table --
def brute_next(dfa, tok_bytes, eos, s):
    """Per token, the DFA state after its bytes from DFA state s (-1: dies)."""
    out = []
    for b in tok_bytes:
        cur = s if b else -1
        for x in b or b"":
            cur = int(dfa.trans[cur, x]) if cur >= 0 else -1
        out.append(cur)
    return out


def check_table(spec, tok_bytes, eos):
    dfa = G.regex_to_dfa(G.spec_to_regex(spec))
    g = G.compile(spec, tok_bytes, eos)
    nxt, (S, V) = g.next, g.next.shape
    assert nxt.dtype == np.int16 and V == len(tok_bytes)
    sink = S - 1
    # table state -> DFA state, discovered from the start by the brute-force walk
    dstate, todo = {0: 0}, [0]
    while todo:
        s = todo.pop()
        ref = brute_next(dfa, tok_bytes, eos, dstate[s])
        for t in range(V):
            if t in eos:
                want_eos = sink if dfa.accept[dstate[s]] else -1
                assert nxt[s, t] == want_eos, (s, t)
                continue
            if nxt[s, t] < 0:
                continue
            assert ref[t] >= 0 and tok_bytes[t], (s, t)  # never a None / empty token, never a dead walk
            d = int(nxt[s, t])
            assert 0 <= d < sink
            if d in dstate:
                assert dstate[d] == ref[t], (s, t)
            else:
                dstate[d] = ref[t]
                todo.append(d)
        # a token the table refuses either dies in the DFA or leads where no accepting state can be
        # reached by whole tokens; over a vocabulary with every single byte nothing is dropped
        if all(bytes([b]) in tok_bytes for b in range(256)):
            assert [t for t in range(V) if t not in eos and nxt[s, t] < 0 and ref[t] >= 0] == []
    assert sorted(dstate) == list(range(sink))  # only states reachable by tokens are kept
    assert (nxt[:sink] >= 0).any(1).all()       # every kept state allows a token
    assert [t for t in range(V) if nxt[sink, t] >= 0] == sorted(eos) and (nxt[sink, sorted(eos)] == sink).all()
    return g


SPECS = [{"choice": ["yes", "no", "maybe"]}, {"regex": r"[0-9]{3}-[a-f]{2}"}, {"regex": r"(ab|a)*c.é?"},
         {"json_schema": {"type": "object", "properties": {"ok": {"type": "boolean"}, "n": {"enum": [1, 22, "x"]}}}}]


@pytest.mark.parametrize("spec", SPECS)
def test_token_table_byte_tokenizer(spec):
    tb = G.token_bytes(ByteTokenizer(), 300)
    assert tb[:3] == [None] * 3 and tb[3] == b"\x00" and tb[258] == b"\xff" and tb[259:] == [None] * 41
    check_table(spec, tb, {1, 2})


@pytest.fixture(scope="module")
def bpe(tmp_path_factory):
    """A small byte-level BPE trained in the test on an in-test corpus, with special tokens."""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, trainers

    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    corpus = ['{"ok": true, "n": 22}', "yes no maybe yes no", "123-ab 456-cd 789-ef", "abababac xé", "hello world é日本"] * 4
    tr = trainers.BpeTrainer(vocab_size=330, special_tokens=["<s>", "</s>"],
                             initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False)
    tok.train_from_iterator(corpus, tr)
    path = tmp_path_factory.mktemp("bpe") / "tokenizer.json"
    tok.save(str(path))
    return HFTokenizer(path)


@pytest.mark.parametrize("spec", SPECS)
def test_token_table_byte_level_bpe(bpe, spec):
    n = bpe._tok.get_vocab_size()
    tb = G.token_bytes(bpe, n + 7)  # 7 ids of model padding
    assert tb[0] is None and tb[1] is None and tb[n:] == [None] * 7  # specials and padding
    assert len({b for b in tb if b and len(b) == 1}) == 256 and any(len(b) > 1 for b in tb if b)
    for i in range(2, n):  # the bytes are what the tokenizer decodes the id to
        assert tb[i] == bpe._tok.decode([i]).encode("utf-8") or b"\xef\xbf\xbd" in bpe._tok.decode([i]).encode("utf-8")
    g = check_table(spec, tb, {1})
    assert (g.next[:, 0] < 0).all() and (g.next[:, n:] < 0).all()


def test_token_bytes_sentencepiece_style_and_unknown(tmp_path):
    from tokenizers import Tokenizer, decoders, models

    vocab = {"<unk>": 0, "<s>": 1, "</s>": 2, "<0x41>": 3, "<0xC3>": 4, "▁hello": 5, "wor▁ld": 6, "é": 7}
    tok = Tokenizer(models.BPE(vocab, [], unk_token="<unk>", byte_fallback=True))
    tok.decoder = decoders.Sequence([decoders.Replace("▁", " "), decoders.ByteFallback(), decoders.Fuse()])
    tok.add_special_tokens(["<unk>", "<s>", "</s>"])
    tok.save(str(tmp_path / "tokenizer.json"))
    tb = G.token_bytes(HFTokenizer(tmp_path / "tokenizer.json"), 10)
    assert tb == [None, None, None, b"A", b"\xc3", b" hello", b"wor ld", "é".encode(), None, None]
    tok.decoder = decoders.WordPiece()
    tok.save(str(tmp_path / "tokenizer.json"))
    with pytest.raises(ValueError, match="decoder"):
        G.token_bytes(HFTokenizer(tmp_path / "tokenizer.json"), 10)


def test_compile_errors():
    tb = G.token_bytes(ByteTokenizer(), 300)
    with pytest.raises(ValueError, match="states"):
        G.compile({"regex": "[0-9]{40}"}, tb, [1], max_states=16)
    assert G.compile({"regex": "[0-9]{40}"}, tb, [1], max_states=42).num_states == 42
    digits_only = [None] * 3 + [bytes([b]) if 0x30 <= b <= 0x39 else None for b in range(256)]
    with pytest.raises(ValueError, match="empty"):
        G.compile({"regex": "[a-z]+"}, digits_only, [1])        # no token spells a member
    with pytest.raises(ValueError, match="empty"):
        G.compile({"regex": "[0-9]+x"}, digits_only, [1])       # ... or reaches an accepting state
    g = G.compile({"regex": "[0-9]+x?"}, digits_only, [1])      # the dead branch is cut, the rest kept
    assert g.num_states == 3 and g.next[1, 3 + ord("x")] < 0
    with pytest.raises(ValueError, match="EOS"):
        G.compile({"regex": "a"}, tb, [])
    for bad in ({"choice": []}, {"choice": ["a", ""]}, {"choice": "yes"}, {"regex": ""}, {"regex": 3},
                {"choice": ["a"], "regex": "a"}, {"ebnf": "x"}, {}):
        with pytest.raises(ValueError):
            G.compile(bad, tb, [1])


def test_reference_functions():
    nxt = np.array([[1, -1, 0, -1], [-1, -1, 1, 2], [-1, -1, -1, 2]], np.int16)
    arena = torch.full((8, 8), -1, dtype=torch.int16)
    arena[3:6, :4] = torch.from_numpy(nxt)
    logits = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    state = torch.tensor([1, 0, 2, 0], dtype=torch.int32)
    out = G.mask_reference(logits.clone(), arena, [3, -1, 3], state, rows=[2, 1, 0])
    ninf = float("-inf")
    assert out.tolist() == [[ninf, ninf, ninf, 3.0], [4.0, 5.0, 6.0, 7.0], [ninf, ninf, 10.0, 11.0]]
    G.advance_reference(arena, [3, -1, 3, 3], state, torch.tensor([3, 0, 2, 99]), rows=[2, 1, 0, 3], vocab=4)
    # row 2: state 2 -> 2; row 1 unguided; row 0: state 1 -> 1; row 3: token 99 clamps to 3: not allowed, kept
    assert state.tolist() == [1, 0, 2, 0]
    G.advance_reference(arena, [3], state, torch.tensor([-5]), rows=[3], vocab=4)  # clamps to 0: state 0 -> 1
    assert state.tolist() == [1, 0, 2, 1]


# ------------------------------------------------------------------ JSON schema --
SCHEMAS = [
    {"type": "object", "properties": {"name": {"type": "string", "maxLength": 6}, "age": {"type": "integer"}}},
    {"type": "array", "items": {"type": "number"}, "minItems": 1, "maxItems": 4},
    {"type": "array", "items": {"enum": ["red", "green", 3, None, True, 1.5]}},
    {"type": "object", "properties": {"a": {"type": "object", "properties": {
        "b": {"type": "array", "items": {"type": "object", "properties": {"c": {"type": "boolean"}}}, "maxItems": 2}}},
        "z": {"type": "null"}}},
    {"type": "string", "minLength": 2, "maxLength": 5},
    {"type": "object", "properties": {"id": {"type": "string", "pattern": "^[A-Z]{2}-[0-9]{3}$"}, "k": {"const": "v\"q"}}},
    {"type": "array", "items": {"type": "array", "items": {"type": "integer"}, "minItems": 2, "maxItems": 2}, "minItems": 2},
    {"type": "object", "properties": {}, "additionalProperties": False},
    {"enum": ["a b", "c\\d", 7]},
]


def conforms(v, sch):
    if "enum" in sch or "const" in sch:
        vals = [sch["const"]] if "const" in sch else sch["enum"]
        return any(v == x and type(v) is type(x) for x in vals)
    t = sch["type"]
    if t == "string":
        ok = isinstance(v, str) and sch.get("minLength", 0) <= len(v) <= sch.get("maxLength", 10**9)
        return ok and ("pattern" not in sch or re.fullmatch(sch["pattern"].strip("^$"), v) is not None)
    if t == "integer":
        return isinstance(v, int) and not isinstance(v, bool)
    if t == "number":
        return isinstance(v, (int, float)) and not isinstance(v, bool)
    if t == "boolean":
        return isinstance(v, bool)
    if t == "null":
        return v is None
    if t == "array":
        return (isinstance(v, list) and sch.get("minItems", 0) <= len(v) <= sch.get("maxItems", 10**9)
                and all(conforms(x, sch["items"]) for x in v))
    props = sch.get("properties", {})
    return isinstance(v, dict) and list(v) == list(props) and all(conforms(v[k], s) for k, s in props.items())


@pytest.mark.parametrize("idx", range(len(SCHEMAS)))
def test_json_schema_random_walks_parse_and_conform(idx):
    sch = SCHEMAS[idx]
    dfa = G.regex_to_dfa(G.schema_to_regex(sch))
    n = dfa.trans.shape[0]
    # distance to the nearest accepting state, to steer a walk home after enough random steps
    dist = np.where(dfa.accept, 0, 10**9)
    for _ in range(n):
        step = np.where(dfa.trans >= 0, dist[np.maximum(dfa.trans, 0)] + 1, 10**9).min(1)
        dist = np.minimum(dist, step)
    rng = random.Random(idx)
    for _ in range(40):
        s, out, budget = 0, bytearray(), rng.randrange(4, 60)
        while True:
            if dfa.accept[s] and (len(out) >= budget or not (dfa.trans[s] >= 0).any()):
                break
            allowed = np.nonzero(dfa.trans[s] >= 0)[0].tolist()
            if len(out) >= budget:  # head for an accepting state
                allowed = [b for b in allowed if dist[dfa.trans[s, b]] < dist[s]]
            b = rng.choice(allowed)
            out.append(b)
            s = int(dfa.trans[s, b])
        text = out.decode("utf-8")  # every path is well-formed UTF-8
        assert conforms(json.loads(text), sch), text
    # the canonical serialisations, with and without the optional spaces, are members
    assert G.schema_to_regex(json.dumps(sch)) == G.schema_to_regex(sch)


@pytest.mark.parametrize("schema,keyword", [
    ({"$ref": "#/x"}, r"\$ref"), ({"anyOf": [{"type": "null"}]}, "anyOf"), ({"oneOf": []}, "oneOf"),
    ({"allOf": []}, "allOf"), ({"type": "object", "patternProperties": {}}, "patternProperties"),
    ({"type": "object", "additionalProperties": True}, "additionalProperties"),
    ({"type": "object", "additionalProperties": {"type": "string"}}, "additionalProperties"),
    ({"type": "integer", "minimum": 3}, "minimum"), ({"type": "string", "format": "date"}, "format"),
    ({"type": ["string", "null"]}, "type"), ({}, "type"), ({"type": "array"}, "items"),
    ({"type": "string", "pattern": "a.*"}, "pattern"), ({"type": "string", "pattern": "(?=a)"}, "look-around"),
    ({"enum": [[1]]}, "scalars"), ({"type": "object", "properties": {"a": {"$ref": "#"}}}, r"\$ref"),
])
def test_json_schema_unsupported_raises(schema, keyword):
    with pytest.raises(ValueError, match=keyword):
        G.schema_to_regex(schema)


# ------------------------------------------------------------------ engine --
BIG = replace(TINY_LLAMA, name="tiny-llama-guided")  # vocab 512 >= 259: the byte tokenizer fits
assert BIG.vocab_size >= 259
TOK = ByteTokenizer()
OBJ = {"type": "object", "properties": {"ok": {"type": "boolean"}, "n": {"enum": [1, 22]}}}
# bounded languages only: (spec, full-match regex of the decoded output, longest member in bytes)
GRAMMARS = [({"choice": ["yes", "no", "maybe"]}, r"yes|no|maybe", 5),
            ({"regex": r"[0-9]{3}-[a-f]{2}"}, r"[0-9]{3}-[a-f]{2}", 6),
            ({"json_schema": OBJ}, r'\{"ok": ?(true|false), ?"n": ?(1|22)\}', 22)]
SAMPLING = [dict(), dict(temperature=1.5, seed=11), dict(temperature=1.5, seed=5, top_k=2)]
_MODEL = []


def model():
    if not _MODEL:
        torch.manual_seed(0)
        _MODEL.append(build_model(BIG, device="cpu", dtype=torch.float32, seed=3))
    return _MODEL[0]


def engine(asy=False, tokenizer=True, **kw):
    cfg = dict(max_num_seqs=8, max_num_batched_tokens=64, max_model_len=128, num_kv_blocks=64, use_graphs=False,
               async_scheduling=asy, grammar_states=128)
    cfg.update(kw)
    eng = Engine(model(), EngineConfig(**cfg))
    if tokenizer and cfg["grammar_states"]:
        eng.set_tokenizer(TOK)
    return eng


def run(eng, reqs):
    """[(prompt, params)] -> [(tokens, finish reason)] in request order."""
    seqs = [eng.add_request(p, sp) for p, sp in reqs]
    for _ in range(2000):
        if not eng.has_work():
            break
        eng.step()
    assert not eng.has_work()
    return [(list(s.output), s.finish_reason) for s in seqs]


def guided_requests(extra=0):
    reqs, want = [], []
    for i, ((spec, rx, longest), samp) in enumerate(itertools.product(GRAMMARS, SAMPLING)):
        reqs.append(([5 + i, 9, 40 + i], SamplingParams(max_tokens=longest + 2 + extra, guided=spec, **samp)))
        want.append(rx)
    return reqs, want


def assert_full_matches(outs, want):
    for (toks, reason), rx in zip(outs, want):
        assert reason == "stop", (reason, TOK.decode(toks))  # a "length" finish is a failure
        assert toks[-1] == BIG.eos_token_id and all(3 <= t < 259 for t in toks[:-1])
        text = TOK.decode(toks[:-1])
        assert re.fullmatch(rx, text), (rx, text)


def test_engine_guided_outputs_match_sync_and_async():
    reqs, want = guided_requests()
    out_sync = run(engine(False), reqs)
    assert_full_matches(out_sync, want)
    eng = engine(True)
    out_async = run(eng, reqs)
    assert out_async == out_sync
    assert eng.stats["guided_rows"] > 0 and eng.stats["grammar_arena_bytes"] == 128 * 512 * 2
    assert eng.stats["grammar_uploads"] == len(GRAMMARS)  # one upload per grammar, shared by its requests
    assert all(g.refs == 0 for g in eng._g_resident) and (eng.r_gbase == -1).all()


@pytest.mark.parametrize("asy", [False, True])
def test_engine_unguided_requests_unchanged_in_a_mixed_batch(asy):
    plain = [([7, 8, 9, 10 + i], SamplingParams(max_tokens=12, ignore_eos=True, **samp))
             for i, samp in enumerate([dict(), dict(temperature=0.9, seed=3), dict(temperature=1.2, seed=4, top_k=5),
                                       dict(repetition_penalty=1.3), dict(logprobs=2)])]
    alone = run(engine(asy, grammar_states=0), plain)
    greqs, want = guided_requests()
    mixed = [plain[0], greqs[0], plain[1], greqs[4], plain[2], plain[3], greqs[8], plain[4]]
    outs = run(engine(asy), mixed)
    assert [outs[i] for i in (0, 2, 4, 5, 7)] == alone
    assert_full_matches([outs[i] for i in (1, 3, 6)], [want[0], want[4], want[8]])


@pytest.mark.parametrize("asy", [False, True])
def test_engine_preemption_and_readmission(asy):
    reqs, want = guided_requests()
    # 15-token prompts: one page at admission, a second one with the first tokens, for 8 rows at once
    reqs = [(list(range(5, 5 + 12)) + p, sp) for p, sp in reqs]
    eng = engine(asy, num_kv_blocks=11, enable_prefix_caching=False, max_num_batched_tokens=256)
    outs = run(eng, reqs)
    assert eng.stats["preemptions"] > 0
    assert_full_matches(outs, want)
    assert outs == run(engine(asy, max_num_batched_tokens=256), reqs)  # and the tokens are those of an engine that never preempted


def test_engine_small_arena_waits_evicts_and_uploads():
    gs = [G.compile(spec, G.token_bytes(TOK, BIG.vocab_size), BIG.eos_ids) for spec, _, _ in GRAMMARS]
    sizes = [g.num_states for g in gs]
    reqs, want = guided_requests()
    # room for the largest grammar alone: two live grammars never fit
    eng = engine(False, grammar_states=max(sizes))
    outs = run(eng, reqs)
    assert_full_matches(outs, want)
    assert eng.stats["grammar_evictions"] >= 2 and eng.stats["grammar_uploads"] >= 3
    assert outs == run(engine(False), reqs)
    # a grammar larger than the arena is refused at the request, not in the step loop
    with pytest.raises(ValueError, match="states"):
        engine(False, grammar_states=min(sizes)).check_request([5], SamplingParams(guided=GRAMMARS[2][0]))
    # the host cache keeps grammar_cache grammars
    eng = engine(False, grammar_cache=2)
    for spec, _, _ in GRAMMARS:
        eng.check_request([5], SamplingParams(guided=spec))
    assert len(eng._g_cache) == 2
    g = eng.compile_guided(SamplingParams(guided=GRAMMARS[2][0]))
    assert eng.compile_guided(SamplingParams(guided={"json_schema": json.dumps(OBJ)})) is g  # same canonical spec


def test_engine_check_request_errors():
    sp = SamplingParams(guided={"choice": ["a", "b"]})
    with pytest.raises(ValueError, match="grammar_states = 0"):
        engine(grammar_states=0).check_request([5], sp)
    with pytest.raises(ValueError, match="tokenizer"):
        engine(tokenizer=False).check_request([5], sp)
    eng = engine()
    eng.check_request([5], sp)
    with pytest.raises(ValueError, match="ignore_eos"):
        eng.check_request([5], SamplingParams(guided={"choice": ["a"]}, ignore_eos=True))
    with pytest.raises(ValueError, match="exactly one"):
        eng.check_request([5], SamplingParams(guided={"choice": ["a"], "regex": "a"}))
    with pytest.raises(ValueError, match="exactly one"):
        SamplingParams(guided={"grammar": "x"}).validate()
    with pytest.raises(ValueError, match="look-around"):
        eng.check_request([5], SamplingParams(guided={"regex": "(?=a)b"}))
    with pytest.raises(ValueError, match="grammar_states"):
        engine(grammar_states=40000)
    # tensor / expert parallel engines are rejected at construction, EP predictors at the request
    from types import SimpleNamespace

    from mlopamd.runtime.ep_serving import check_ep_request

    for tp, ep in ((2, 1), (1, 4)):
        sharded = SimpleNamespace(**vars(model()))
        sharded.ps = SimpleNamespace(tp=SimpleNamespace(size=tp), ep=SimpleNamespace(size=ep))
        with pytest.raises(ValueError, match="tensor or expert parallelism"):
            Engine(sharded, EngineConfig(max_num_seqs=2, max_model_len=64, num_kv_blocks=8, use_graphs=False,
                                         grammar_states=8))
    with pytest.raises(ValueError, match="guided"):
        check_ep_request(sp)
    assert SamplingParams(guided={"regex": "a"}).extended and not SamplingParams().extended
    assert "grammar_arena_bytes" not in engine(grammar_states=0).stats


# ------------------------------------------------------------------ server --
def test_server_guided_parameters_and_errors():
    from aiohttp.test_utils import TestClient, TestServer

    from mlopamd.runtime.metrics import RuntimeMetrics
    from mlopamd.runtime.server import make_app

    backend = LLMBackend(engine(True), RuntimeMetrics("llm", "v1", "ns", "tiny"), name="tiny").start()
    off = LLMBackend(engine(True, grammar_states=0), None, name="off")

    async def go():
        async with TestClient(TestServer(make_app(backend, backend.metrics))) as c:
            async def gen(params, expect=200):
                r = await c.post("/v2/models/tiny/generate", json={"text_input": "q", "parameters": params})
                assert r.status == expect, (params, r.status, await r.text())
                return await r.json() if expect == 200 else None

            b = await gen({"guided_choice": ["yes", "no", "maybe"], "max_tokens": 8})
            assert b["text_output"] in ("yes", "no", "maybe") and b["finish_reason"] == "stop"
            b = await gen({"guided_regex": "[0-9]{3}-[a-f]{2}", "max_tokens": 9, "temperature": 1.5, "seed": 1})
            assert re.fullmatch("[0-9]{3}-[a-f]{2}", b["text_output"]) and b["finish_reason"] == "stop"
            for schema in (OBJ, json.dumps(OBJ)):
                b = await gen({"guided_json": schema, "max_tokens": 30})
                assert b["finish_reason"] == "stop" and conforms(json.loads(b["text_output"]), OBJ)
            md = await (await c.get("/v2/models/tiny")).json()
            assert md["guided_decoding"] is True and md["grammar_arena_bytes"] == 128 * 512 * 2
            bad = [{"guided_choice": ["a"], "guided_regex": "a"}, {"guided_choice": "a"}, {"guided_choice": []},
                   {"guided_choice": ["a", 3]}, {"guided_regex": 5}, {"guided_regex": "(a"}, {"guided_regex": "a*?"},
                   {"guided_json": "{not json"}, {"guided_json": [1]}, {"guided_json": {"$ref": "#"}},
                   {"guided_json": {"type": "string", "maxLength": 10**6}}, {"guided_regex": "[a-z]{900}[0-9]{900}"},
                   {"guided_choice": ["a"], "ignore_eos": True}]
            for params in bad:
                await gen(params, expect=400)
            b = await gen({"guided_choice": ["yes", "no"], "max_tokens": 8})  # still serving
            assert b["text_output"] in ("yes", "no")
        async with TestClient(TestServer(make_app(off, None))) as c:
            r = await c.post("/v2/models/off/generate", json={"text_input": "q", "parameters": {"guided_regex": "a"}})
            assert r.status == 400 and "grammar_states" in await r.text()
            assert "guided_decoding" not in await (await c.get("/v2/models/off")).json()

    try:
        asyncio.run(go())
    finally:
        backend.stop()


# ------------------------------------------------------------------ CR --
def test_crd_field_operator_env_and_engine_config(monkeypatch):
    import yaml

    from mlopamd.controller import seldon
    from mlopamd.controller.crd import ModelSpec
    from mlopamd.controller.placement import plan
    from mlopamd.runtime.server import engine_kwargs_from_env

    base = {"modelName": "m", "modelAlias": "champion"}
    assert ModelSpec.from_spec(base).guided_decoding_states is None and ModelSpec.from_spec(base).validate() == []
    assert ModelSpec.from_spec({**base, "guidedDecodingStates": 4096}).validate() == []
    assert ModelSpec.from_spec({**base, "guidedDecodingStates": 0, "tensorParallel": 8}).validate() == []
    for bad in (-1, 32768, "64", True, 1.5):
        assert any("guidedDecodingStates" in e for e in ModelSpec.from_spec({**base, "guidedDecodingStates": bad}).validate())
    for par in ({"tensorParallel": 2}, {"expertParallel": 4}):
        errs = ModelSpec.from_spec({**base, "guidedDecodingStates": 64, **par}).validate()
        assert any("guidedDecodingStates" in e and "tensorParallel" in e for e in errs)
    with open("manifests/crd.yaml") as f:
        crd = yaml.safe_load(f)
    props = crd["spec"]["versions"][0]["schema"]["openAPIV3Schema"]["properties"]["spec"]["properties"]
    assert props["guidedDecodingStates"]["type"] == "integer"
    assert (props["guidedDecodingStates"]["minimum"], props["guidedDecodingStates"]["maximum"]) == (0, 32767)
    with open("manifests/examples/guided/llama3-8b-guided.yaml") as f:
        ex = yaml.safe_load(f)
    spec = ModelSpec.from_spec(ex["spec"])
    assert spec.validate() == [] and spec.guided_decoding_states == 4096
    # the operator's env var, as it emits MLOP_ENGINE_SPEC_TOKENS, and the runtime reading it back
    pred = seldon.build_predictor("1", "s3://mlflow/x", None, 100, runtime=seldon.RUNTIME_LLM, replicas=1,
                                  placement=None, image="img", gpu_resource="amd.com/gpu", model_name="m",
                                  deployment="d", namespace="ns", architecture="llama3-8b",
                                  engine_args={"grammar_states": spec.guided_decoding_states})
    env = {e["name"]: e["value"] for e in json.loads(json.dumps(pred))["componentSpecs"][0]["spec"]["containers"][0]["env"]}
    assert env["MLOP_ENGINE_GRAMMAR_STATES"] == "4096"
    monkeypatch.setenv("MLOP_ENGINE_GRAMMAR_STATES", env["MLOP_ENGINE_GRAMMAR_STATES"])
    kw = engine_kwargs_from_env()
    assert kw["grammar_states"] == 4096 and EngineConfig(**kw).grammar_states == 4096
    # placement charges states x vocab x 2 bytes
    a, b = plan("llama3-8b"), plan("llama3-8b", grammar_states=4096)
    assert a.kvTokenCapacity > b.kvTokenCapacity
    assert abs((a.kvGBPerGPU - b.kvGBPerGPU) - 4096 * 128256 * 2 / 1e9) < 0.011
