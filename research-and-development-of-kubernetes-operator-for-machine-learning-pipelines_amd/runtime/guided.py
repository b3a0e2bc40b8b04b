"""Guided decoding (K18): regex, choice and JSON-schema constraints compiled to a per-grammar
token-transition table.

Host side, pure Python + NumPy, run in the caller's thread (``Engine.check_request``), never in
the step loop:

  spec -> regex -> Thompson NFA over UTF-8 BYTES -> subset construction -> trim (+ Moore
  minimisation) -> byte DFA -> ``Grammar.next``: int16 [S, V], entry [s, t] = the state after
  walking token t's bytes from state s, -1 = token t is not allowed in state s.

State 0 is the start; only states reachable by whole tokens are kept.  In an accepting state
every EOS id leads to the final sink state (the last one), which allows exactly the EOS ids and
stays in itself; everywhere else the EOS ids are -1.  The device side is ops/csrc/guided.hip
(``ops.grammar_mask`` / ``ops.grammar_advance``); ``mask_reference`` / ``advance_reference``
below are the contract those kernels are held to.

Regex subset (full match, no anchors): literals and escapes (\\d \\w \\s \\n \\t \\r \\f \\v
\\\\ \\xNN, escaped punctuation), ``.`` (any character but \\n), classes ``[...]`` / ``[^...]`` with
ASCII ranges, groups ``( )`` / ``(?: )``, ``|``, ``* + ? {m} {m,} {m,n}``.  \\d \\w \\s are the
ASCII sets.  ``.`` and negated classes also accept every well-formed 2-4 byte UTF-8 sequence.
Everything else raises ValueError naming the construct.
"""
from __future__ import annotations

import hashlib
import json
import re as _re

import numpy as np

MAX_STATES = 32767      # int16 table entries
MAX_REPEAT = 1024       # largest bound of a {m,n} quantifier
_NFA_LIMIT = 200_000    # NFA states of one pattern (nested bounded repeats multiply)

_DIGIT = frozenset(range(0x30, 0x3A))
_WORD = frozenset([*range(0x30, 0x3A), *range(0x41, 0x5B), *range(0x61, 0x7B), 0x5F])
_SPACE = frozenset([0x20, 0x09, 0x0A, 0x0D, 0x0C, 0x0B])
_ASCII = frozenset(range(0x80))
_CONT = frozenset(range(0x80, 0xC0))
# every well-formed non-ASCII UTF-8 sequence (no overlongs, no surrogates, <= U+10FFFF)
_UTF8_SEQS = (
    (range(0xC2, 0xE0), _CONT),
    ((0xE0,), range(0xA0, 0xC0), _CONT),
    ((*range(0xE1, 0xED), 0xEE, 0xEF), _CONT, _CONT),
    ((0xED,), range(0x80, 0xA0), _CONT),
    ((0xF0,), range(0x90, 0xC0), _CONT, _CONT),
    (range(0xF1, 0xF4), _CONT, _CONT, _CONT),
    ((0xF4,), range(0x80, 0x90), _CONT, _CONT),
)
_ESC_CHAR = {"n": 0x0A, "t": 0x09, "r": 0x0D, "f": 0x0C, "v": 0x0B}
_ESC_SET = {"d": _DIGIT, "w": _WORD, "s": _SPACE}
_META = set("\\.[](){}|*+?^$")


# ------------------------------------------------------------------ regex -> AST --
class _Char:
    """One character: a set of ASCII bytes, literal non-ASCII characters (their UTF-8 bytes)
    and / or "any non-ASCII character"."""

    __slots__ = ("ascii", "multi", "any_multi")

    def __init__(self, ascii_=(), multi=(), any_multi=False):
        self.ascii, self.multi, self.any_multi = frozenset(ascii_), tuple(multi), any_multi


class _Parser:
    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise ValueError(f"regex must be a string, got {type(pattern).__name__}")
        self.p, self.i = pattern, 0

    def fail(self, what: str):
        raise ValueError(f"unsupported regex construct: {what} (at offset {self.i} of {self.p!r})")

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.peek() not in "|)":
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self):
        atom = self.atom()
        while True:
            c = self.peek()
            if c == "*":
                lo, hi = 0, None
            elif c == "+":
                lo, hi = 1, None
            elif c == "?":
                lo, hi = 0, 1
            elif c == "{":
                m = _re.compile(r"\{(\d+)(?:(,)(\d*))?\}").match(self.p, self.i)
                if m is None:
                    if _re.compile(r"\{,\d*\}").match(self.p, self.i):
                        self.fail("quantifier without a lower bound '{,n}'")
                    return atom  # a literal '{': the next atom
                lo = int(m.group(1))
                hi = lo if m.group(2) is None else (int(m.group(3)) if m.group(3) else None)
                if hi is not None and hi < lo:
                    self.fail(f"quantifier {m.group(0)} with max < min")
                if max(lo, hi or 0) > MAX_REPEAT:
                    self.fail(f"quantifier bound above {MAX_REPEAT}")
                self.i = m.end() - 1
            else:
                return atom
            self.i += 1
            if self.peek() == "?":
                self.fail("lazy quantifier")
            if self.peek() == "+":
                self.fail("possessive quantifier")
            atom = ("rep", atom, lo, hi)

    def atom(self):
        c = self.peek()
        if c == "(":
            self.i += 1
            if self.peek() == "?":
                nxt = self.p[self.i + 1:self.i + 3]
                if nxt[:1] == ":":
                    self.i += 2
                elif nxt[:1] in ("=", "!") or nxt in ("<=", "<!"):
                    self.fail("look-around")
                elif nxt[:1] == "P" or nxt[:1] == "<":
                    self.fail("named group / backreference")
                else:
                    self.fail(f"group extension '(?{nxt[:1]}'")
            node = self.alt()
            if self.peek() != ")":
                self.fail("unbalanced '('")
            self.i += 1
            return node
        if c in "*+?":
            self.fail(f"quantifier '{c}' with nothing to repeat")
        if c in "^$":
            self.fail(f"anchor '{c}' (the match is anchored at both ends already)")
        if c == "[":
            return self.klass()
        if c == ".":
            self.i += 1
            return _Char(_ASCII - {0x0A}, any_multi=True)
        if c == "\\":
            return self.escape(in_class=False)
        self.i += 1
        return self.literal(c)

    @staticmethod
    def literal(ch: str):
        b = ch.encode("utf-8")
        return _Char(b) if len(b) == 1 else _Char(multi=[b])

    def escape(self, in_class: bool):
        self.i += 1
        c = self.peek()
        if not c:
            self.fail("trailing backslash")
        self.i += 1
        if c in _ESC_SET:
            return _Char(_ESC_SET[c])
        if c in _ESC_CHAR:
            return _Char([_ESC_CHAR[c]])
        if c == "x":
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or any(d not in "0123456789abcdefABCDEF" for d in h):
                self.fail("malformed \\xNN escape")
            self.i += 2
            return self.literal(chr(int(h, 16)))
        if c.isdigit() and not in_class:
            self.fail("backreference")
        if c in "AZbBG" and not in_class:
            self.fail(f"anchor '\\{c}'")
        if c.isalnum():
            self.fail(f"escape '\\{c}'")
        return self.literal(c)

    def klass(self):
        self.i += 1
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        ascii_, multi, first = set(), [], True
        while True:
            c = self.peek()
            if not c:
                self.fail("unterminated character class")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            if c == "[" and self.p[self.i + 1:self.i + 2] in (":", ".", "="):
                self.fail("named character class")
            if c == "\\":
                lo = self.escape(in_class=True)
            else:
                self.i += 1
                lo = self.literal(c)
            single = len(lo.ascii) == 1 and not lo.multi
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                c2 = self.peek()
                if c2 == "\\":
                    hi = self.escape(in_class=True)
                else:
                    self.i += 1
                    hi = self.literal(c2)
                if not single or len(hi.ascii) != 1 or hi.multi:
                    self.fail("class range with a non-ASCII or multi-character endpoint")
                a, b = next(iter(lo.ascii)), next(iter(hi.ascii))
                if b < a:
                    self.fail("class range with end < start")
                ascii_.update(range(a, b + 1))
                continue
            ascii_ |= lo.ascii
            multi.extend(lo.multi)
        if negate:
            if multi:
                self.fail("non-ASCII character in a negated class")
            return _Char(_ASCII - ascii_, any_multi=True)
        return _Char(ascii_, multi)


# ------------------------------------------------------------------ AST -> NFA -> DFA --
class _NFA:
    def __init__(self):
        self.eps: list[list[int]] = []
        self.edges: list[list[tuple[int, int]]] = []  # per state: (byte-set id, target)
        self.sets: dict[frozenset, int] = {}

    def state(self) -> int:
        if len(self.eps) >= _NFA_LIMIT:
            raise ValueError(f"regex too large: more than {_NFA_LIMIT} NFA states (nested bounded repeats)")
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def edge(self, a: int, byteset, b: int):
        fs = frozenset(byteset)
        if fs:
            self.edges[a].append((self.sets.setdefault(fs, len(self.sets)), b))

    def build(self, node) -> tuple[int, int]:
        """Thompson fragment (start, end) of an AST node."""
        if isinstance(node, _Char):
            s, e = self.state(), self.state()
            self.edge(s, node.ascii, e)
            seqs = [tuple((b,) for b in m) for m in node.multi]
            if node.any_multi:
                seqs.extend(_UTF8_SEQS)
            for seq in seqs:
                cur = s
                for k, bs in enumerate(seq):
                    nxt = e if k == len(seq) - 1 else self.state()
                    self.edge(cur, bs, nxt)
                    cur = nxt
            return s, e
        kind = node[0]
        if kind == "cat":
            s = e = self.state()
            for item in node[1]:
                a, b = self.build(item)
                self.eps[e].append(a)
                e = b
            return s, e
        if kind == "alt":
            s, e = self.state(), self.state()
            for br in node[1]:
                a, b = self.build(br)
                self.eps[s].append(a)
                self.eps[b].append(e)
            return s, e
        _, sub, lo, hi = node
        s = e = self.state()
        for _ in range(lo):
            a, b = self.build(sub)
            self.eps[e].append(a)
            e = b
        if hi is None:
            a, b = self.build(sub)
            loop = self.state()
            self.eps[e].append(loop)
            self.eps[loop].append(a)
            self.eps[b].append(loop)
            return s, loop
        end = self.state()
        for _ in range(hi - lo):
            a, b = self.build(sub)
            self.eps[e].append(end)
            self.eps[e].append(a)
            e = b
        self.eps[e].append(end)
        return s, end


class DFA:
    """Byte automaton: ``trans`` int32 [n, 256] (-1: no transition), ``accept`` bool [n], start 0.
    Every state reaches an accepting state."""

    def __init__(self, trans: np.ndarray, accept: np.ndarray):
        self.trans, self.accept = trans, accept

    def matches(self, data) -> bool:
        if isinstance(data, str):
            data = data.encode("utf-8")
        s = 0
        for b in data:
            s = int(self.trans[s, b])
            if s < 0:
                return False
        return bool(self.accept[s])


def _subset(nfa: _NFA, start: int, final: int) -> DFA:
    n = len(nfa.eps)
    # byte classes: bytes no edge set tells apart move together
    member = np.zeros((max(1, len(nfa.sets)), 256), bool)
    for fs, k in nfa.sets.items():
        member[k, list(fs)] = True
    _, first, cls = np.unique(member.T, axis=0, return_index=True, return_inverse=True)
    cls = cls.reshape(-1)
    reps = first.tolist()
    set_cls = [np.nonzero(member[k, reps])[0].tolist() for k in range(member.shape[0])]
    closure: list = [None] * n

    def close(s0: int) -> frozenset:
        if closure[s0] is None:
            seen, stack = {s0}, [s0]
            while stack:
                for t in nfa.eps[stack.pop()]:
                    if t not in seen:
                        seen.add(t)
                        stack.append(t)
            closure[s0] = frozenset(seen)
        return closure[s0]

    d0 = close(start)
    index, order, rows = {d0: 0}, [d0], []
    i = 0
    while i < len(order):
        move: dict[int, set] = {}
        for s in order[i]:
            for k, t in nfa.edges[s]:
                ct = close(t)
                for c in set_cls[k]:
                    move.setdefault(c, set()).update(ct)
        row = np.full(len(reps), -1, np.int32)
        for c, tgt in move.items():
            f = frozenset(tgt)
            j = index.get(f)
            if j is None:
                j = index[f] = len(order)
                order.append(f)
                if j > 4 * _NFA_LIMIT:
                    raise ValueError("regex too large: the byte automaton exceeds the state limit")
            row[c] = j
        rows.append(row)
        i += 1
    tc = np.stack(rows)                      # [n, classes]
    accept = np.array([final in d for d in order], bool)
    # trim: only states that reach an accepting state
    live = accept.copy()
    while True:
        nxt = live | (np.where(tc >= 0, live[np.maximum(tc, 0)], False)).any(1)
        if (nxt == live).all():
            break
        live = nxt
    if not live[0]:
        raise ValueError("the grammar's language is empty")
    tc = np.where((tc >= 0) & live[np.maximum(tc, 0)], tc, -1)
    # Moore minimisation over the live states
    label = np.where(live, accept.astype(np.int64), -1)
    count = 0
    while True:
        sig = np.concatenate([label[:, None], np.where(tc >= 0, label[np.maximum(tc, 0)], -1)], 1)
        _, new = np.unique(sig, axis=0, return_inverse=True)
        new = np.where(live, new.reshape(-1), -1)
        c = len(np.unique(new[live]))
        label = new
        if c == count:
            break
        count = c
    # renumber in order of first appearance in a BFS from the start, start = 0
    ids, queue, trans_rows, acc = {int(label[0]): 0}, [0], [], []
    reps_of = {}
    for s in np.nonzero(live)[0].tolist():
        reps_of.setdefault(int(label[s]), s)
    qi = 0
    while qi < len(queue):
        s = queue[qi]
        row = np.full(len(reps), -1, np.int32)
        for c in np.nonzero(tc[s] >= 0)[0].tolist():
            lab = int(label[tc[s, c]])
            if lab not in ids:
                ids[lab] = len(queue)
                queue.append(reps_of[lab])
            row[c] = ids[lab]
        trans_rows.append(row)
        acc.append(bool(accept[s]))
        qi += 1
    tcm = np.stack(trans_rows)
    return DFA(np.ascontiguousarray(tcm[:, cls]), np.array(acc, bool))


def regex_to_dfa(pattern: str) -> DFA:
    """The trimmed (and minimised) byte DFA of ``pattern``, full match."""
    ast = _Parser(pattern).parse()
    nfa = _NFA()
    s, e = nfa.build(ast)
    return _subset(nfa, s, e)


# ------------------------------------------------------------------ choice / JSON schema --
def regex_escape(text: str) -> str:
    out = []
    for ch in text:
        if ord(ch) < 0x20 or ord(ch) == 0x7F:
            out.append(f"\\x{ord(ch):02x}")
        elif ch.isascii() and not ch.isalnum() and ch not in " _":
            out.append("\\" + ch)
        else:
            out.append(ch)
    return "".join(out)


def choice_to_regex(choices) -> str:
    if not isinstance(choices, (list, tuple)) or not choices:
        raise ValueError("guided choice must be a non-empty list of strings")
    if any(not isinstance(c, str) or not c for c in choices):
        raise ValueError("guided choice must hold non-empty strings only")
    return "|".join(regex_escape(c) for c in choices)


_JSON_CHAR = r'(?:[^"\\\x00-\x1f]|\\(?:["\\/bfnrt]|u[0-9a-fA-F]{4}))'
_JSON_INT = r"-?(?:0|[1-9][0-9]*)"
_JSON_NUM = _JSON_INT + r"(?:\.[0-9]+)?(?:[eE][+\-]?[0-9]+)?"
_IGNORED_KEYS = {"title", "description", "default", "examples", "$schema", "$id", "$comment", "required"}
_TYPE_KEYS = {
    "string": {"minLength", "maxLength", "pattern"},
    "integer": set(), "number": set(), "boolean": set(), "null": set(),
    "object": {"properties", "additionalProperties"},
    "array": {"items", "minItems", "maxItems"},
}


def _bound(schema, key, default):
    v = schema.get(key, default)
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, int) or v < 0:
        raise ValueError(f"JSON schema keyword {key!r} must be a non-negative integer, got {v!r}")
    if v > MAX_REPEAT:
        raise ValueError(f"JSON schema keyword {key!r} above {MAX_REPEAT}")
    return v


def _json_scalar(v) -> str:
    if v is not None and not isinstance(v, (str, int, float, bool)):
        raise ValueError(f"JSON schema enum / const supports JSON scalars only, got {type(v).__name__}")
    return regex_escape(json.dumps(v, ensure_ascii=False))


def _string_pattern(pattern: str) -> str:
    if not isinstance(pattern, str):
        raise ValueError("JSON schema keyword 'pattern' must be a string")
    if pattern.startswith("^"):
        pattern = pattern[1:]
    if pattern.endswith("$") and not pattern.endswith("\\$"):
        pattern = pattern[:-1]
    t = regex_to_dfa(pattern).trans
    bad = [b for b in (*range(0x20), 0x22, 0x5C, *range(0x7F, 0x100)) if (t[:, b] >= 0).any()]
    if bad:
        raise ValueError("JSON schema keyword 'pattern' may only produce printable ASCII other than "
                         f"'\"' and '\\\\' (it admits byte 0x{bad[0]:02x})")
    return f"(?:{pattern})"


def schema_to_regex(schema, _depth: int = 0) -> str:
    """The regex of the canonical serialisation of ``schema``'s instances: no whitespace except
    one optional space after ':' and ','; every declared property, in declared order."""
    if isinstance(schema, str):
        try:
            schema = json.loads(schema)
        except ValueError as e:
            raise ValueError(f"guided JSON schema is not valid JSON: {e}") from None
    if not isinstance(schema, dict):
        raise ValueError(f"a JSON schema must be an object, got {type(schema).__name__}")
    if _depth > 32:
        raise ValueError("JSON schema nested deeper than 32 levels")
    for k in ("$ref", "anyOf", "oneOf", "allOf", "not", "patternProperties", "$defs", "definitions"):
        if k in schema:
            raise ValueError(f"unsupported JSON schema keyword {k!r}")
    if "enum" in schema or "const" in schema:
        extra = set(schema) - _IGNORED_KEYS - {"enum", "const", "type"}
        if extra:
            raise ValueError(f"unsupported JSON schema keyword {sorted(extra)[0]!r}")
        vals = [schema["const"]] if "const" in schema else schema["enum"]
        if not isinstance(vals, list) or not vals:
            raise ValueError("JSON schema keyword 'enum' must be a non-empty list")
        return "(?:" + "|".join(_json_scalar(v) for v in vals) + ")"
    t = schema.get("type")
    if not isinstance(t, str) or t not in _TYPE_KEYS:
        raise ValueError(f"unsupported JSON schema keyword 'type': {t!r} (one of {sorted(_TYPE_KEYS)})")
    extra = set(schema) - _IGNORED_KEYS - _TYPE_KEYS[t] - {"type"}
    if extra:
        raise ValueError(f"unsupported JSON schema keyword {sorted(extra)[0]!r} (type {t!r})")
    if t == "string":
        if "pattern" in schema:
            if "minLength" in schema or "maxLength" in schema:
                raise ValueError("unsupported JSON schema keyword 'minLength' / 'maxLength' beside 'pattern'")
            return '"' + _string_pattern(schema["pattern"]) + '"'
        lo, hi = _bound(schema, "minLength", 0), _bound(schema, "maxLength", None)
        if hi is not None and hi < lo:
            raise ValueError("JSON schema 'maxLength' below 'minLength'")
        q = "*" if (lo == 0 and hi is None) else f"{{{lo},{'' if hi is None else hi}}}"
        return '"' + _JSON_CHAR + q + '"'
    if t == "integer":
        return _JSON_INT
    if t == "number":
        return _JSON_NUM
    if t == "boolean":
        return "(?:true|false)"
    if t == "null":
        return "null"
    if t == "object":
        if schema.get("additionalProperties", False) is not False:
            raise ValueError("unsupported JSON schema keyword 'additionalProperties' (only false)")
        props = schema.get("properties", {})
        if not isinstance(props, dict):
            raise ValueError("JSON schema keyword 'properties' must be an object")
        parts = [_json_scalar(str(k)) + ": ?" + schema_to_regex(v, _depth + 1) for k, v in props.items()]
        return r"\{" + ", ?".join(parts) + r"\}"
    if "items" not in schema:
        raise ValueError("JSON schema type 'array' needs 'items'")
    item = schema_to_regex(schema["items"], _depth + 1)
    lo, hi = _bound(schema, "minItems", 0), _bound(schema, "maxItems", None)
    if hi is not None and hi < lo:
        raise ValueError("JSON schema 'maxItems' below 'minItems'")
    if hi == 0:
        return r"\[\]"
    more = f"(?:, ?{item}){{{max(lo - 1, 0)},{'' if hi is None else hi - 1}}}"
    body = f"{item}{more}"
    return r"\[" + (body if lo > 0 else f"(?:{body})?") + r"\]"


KINDS = ("choice", "regex", "json_schema")


def spec_to_regex(spec: dict) -> str:
    kind, val = check_spec(spec)
    if kind == "choice":
        return choice_to_regex(val)
    if kind == "regex":
        if not isinstance(val, str) or not val:
            raise ValueError("guided regex must be a non-empty string")
        return val
    return schema_to_regex(val)


def check_spec(spec) -> tuple:
    """(kind, value) of a ``SamplingParams.guided`` dict; ValueError unless it has exactly one
    key out of choice / regex / json_schema (shape only)."""
    if not isinstance(spec, dict) or len(spec) != 1 or next(iter(spec)) not in KINDS:
        got = sorted(spec) if isinstance(spec, dict) else type(spec).__name__
        raise ValueError(f"guided must be a dict with exactly one key out of {list(KINDS)}, got {got}")
    return next(iter(spec.items()))


def spec_key(spec: dict) -> str:
    """Cache key: a hash of (kind, canonical spec).  Property order is part of a schema."""
    kind, val = check_spec(spec)
    if kind == "json_schema" and isinstance(val, str):
        try:
            val = json.loads(val)
        except ValueError as e:
            raise ValueError(f"guided JSON schema is not valid JSON: {e}") from None
    try:
        canon = json.dumps([kind, val], separators=(",", ":"), ensure_ascii=True)
    except (TypeError, ValueError) as e:
        raise ValueError(f"guided {kind} is not JSON-serialisable: {e}") from None
    return hashlib.sha256(canon.encode()).hexdigest()


# ------------------------------------------------------------------ token bytes --
def _gpt2_unicode_to_byte() -> dict:
    bs = [*range(ord("!"), ord("~") + 1), *range(0xA1, 0xAD), *range(0xAE, 0x100)]
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(bs, cs)}


def _decoder_types(node, out: set) -> set:
    if isinstance(node, dict):
        if "type" in node:
            out.add(node["type"])
        if node.get("type") == "Replace" and "▁" in json.dumps(node.get("pattern", ""), ensure_ascii=False):
            out.add("Metaspace")
        for v in node.values():
            _decoder_types(v, out)
    elif isinstance(node, list):
        for v in node:
            _decoder_types(v, out)
    return out


def token_bytes(tokenizer, vocab_size: int) -> list:
    """Per token id in [0, vocab_size): the bytes it decodes to, or None (special / added tokens,
    ids the tokenizer does not have: model padding)."""
    out: list = [None] * vocab_size
    off = getattr(tokenizer, "offset", None)
    if off is not None and not hasattr(tokenizer, "_tok"):  # ByteTokenizer
        for b in range(256):
            if b + off < vocab_size:
                out[b + off] = bytes([b])
        return out
    tk = getattr(tokenizer, "_tok", tokenizer)
    if not hasattr(tk, "to_str"):
        raise ValueError(f"guided decoding cannot read the vocabulary of a {type(tokenizer).__name__}")
    spec = json.loads(tk.to_str())
    kinds = _decoder_types(spec.get("decoder"), set())
    added = {int(a["id"]) for a in spec.get("added_tokens") or ()}
    vocab = tk.get_vocab(with_added_tokens=False)
    if "ByteLevel" in kinds:
        u2b = _gpt2_unicode_to_byte()
        for s, i in vocab.items():
            if i < vocab_size and i not in added and all(c in u2b for c in s):
                out[i] = bytes(u2b[c] for c in s)
        return out
    if "Metaspace" in kinds or "ByteFallback" in kinds:
        byte_tok = _re.compile(r"<0x([0-9A-Fa-f]{2})>")
        for s, i in vocab.items():
            if i >= vocab_size or i in added:
                continue
            m = byte_tok.fullmatch(s)
            out[i] = bytes([int(m.group(1), 16)]) if m else s.replace("▁", " ").encode("utf-8")
        return out
    raise ValueError(f"guided decoding does not know the tokenizer's decoder (types {sorted(kinds)}): "
                     "need byte-level BPE or a sentencepiece-style decoder")


# ------------------------------------------------------------------ token table --
class Grammar:
    """A compiled grammar: ``next`` int16 [S, V] on the host, and its engine-side residency
    (``base``: first arena row or -1, ``refs``: admitted rows using it, ``tick``: last use)."""

    __slots__ = ("next", "key", "base", "refs", "tick")

    def __init__(self, next_: np.ndarray, key: str = ""):
        self.next, self.key = next_, key
        self.base, self.refs, self.tick = -1, 0, 0

    @property
    def num_states(self) -> int:
        return self.next.shape[0]

    def walk(self, tokens, state: int = 0) -> int:
        """The state after ``tokens`` (a token the state does not allow leaves it unchanged)."""
        V = self.next.shape[1]
        for t in tokens:
            nx = int(self.next[state, min(max(int(t), 0), V - 1)])
            if nx >= 0:
                state = nx
        return state


def _walk_state(trans: np.ndarray, s: int, B: np.ndarray, lens: np.ndarray, longer: np.ndarray,
                by_first: list) -> np.ndarray:
    """DFA state after each token's bytes from state ``s`` (-1: dies), all tokens at once: one
    gather per byte position over the tokens still alive.  ``B`` [n, Lmax] and ``lens`` are sorted
    by length, longest first; ``longer[p]`` = tokens longer than p; ``by_first[b]`` = the tokens
    whose first byte is b (the walk starts from those whose first byte the state accepts)."""
    n = len(lens)
    res = np.full(n, -1, np.int32)
    first = [by_first[b] for b in np.nonzero(trans[s] >= 0)[0].tolist()]
    alive = np.concatenate(first) if first else np.zeros(0, np.int64)
    cur = np.full(alive.size, s, np.int32)
    for pos in range(B.shape[1]):
        m = alive < longer[pos]
        alive, cur = alive[m], cur[m]
        if not alive.size:
            break
        cur = trans[cur, B[alive, pos]]
        k = cur >= 0
        alive, cur = alive[k], cur[k]
        fin = lens[alive] == pos + 1
        res[alive[fin]] = cur[fin]
    return res


def compile_dfa(dfa: DFA, tok_bytes, eos_ids, max_states: int = MAX_STATES, key: str = "") -> Grammar:
    V = len(tok_bytes)
    eos = sorted({int(e) for e in eos_ids if 0 <= int(e) < V})
    if not eos:
        raise ValueError("guided decoding needs at least one EOS id inside the vocabulary")
    max_states = min(int(max_states), MAX_STATES)
    ids = np.array([i for i, b in enumerate(tok_bytes) if b and i not in eos], np.int64)
    lens = np.array([len(tok_bytes[i]) for i in ids], np.int64)
    order = np.argsort(-lens, kind="stable")
    ids, lens = ids[order], lens[order]
    Lmax = int(lens[0]) if len(lens) else 0
    B = np.zeros((len(ids), max(Lmax, 1)), np.uint8)
    for r, i in enumerate(ids.tolist()):
        b = tok_bytes[i]
        B[r, :len(b)] = np.frombuffer(b, np.uint8)
    longer = np.array([(lens > p).sum() for p in range(max(Lmax, 1))], np.int64)
    by_first = [np.nonzero(B[:, 0] == b)[0] for b in range(256)] if len(ids) else [np.zeros(0, np.int64)] * 256
    # token-level walk from every state reachable by whole tokens; a row is stored as local state
    # ids at once (its successors get their ids when it is walked), and the state graph is kept
    # beside it so that what follows never scans the [states, tokens] matrix more than once
    index, queue, rows, succ = {0: 0}, [0], [], []
    lut = np.full(dfa.trans.shape[0] + 1, -1, np.int16)  # DFA state -> local id (lut[-1] = -1: dead)
    lut[0] = 0
    qi = 0
    while qi < len(queue):
        res = _walk_state(dfa.trans, queue[qi], B, lens, longer, by_first)
        out = np.unique(res[res >= 0]).tolist()
        for d in out:
            if d not in index:
                index[d] = lut[d] = len(queue)
                queue.append(d)
                if len(queue) + 1 > max_states:
                    raise ValueError(f"grammar needs more than {max_states} states")
        rows.append(lut[res])
        succ.append([index[d] for d in out])
        qi += 1
    n = len(queue)
    acc = dfa.accept[np.array(queue)]
    # keep only states from which an accepting state is reachable by TOKENS ...
    pred = [[] for _ in range(n)]
    for a, outs in enumerate(succ):
        for d in outs:
            pred[d].append(a)
    good = acc.copy()
    stack = np.nonzero(acc)[0].tolist()
    while stack:
        for a in pred[stack.pop()]:
            if not good[a]:
                good[a] = True
                stack.append(a)
    if not good[0]:
        raise ValueError("the grammar's language is empty over this vocabulary")
    # ... that the start still reaches through such states
    seen, stack = {0}, [0]
    while stack:
        for d in succ[stack.pop()]:
            if good[d] and d not in seen:
                seen.add(d)
                stack.append(d)
    keep = sorted(seen)
    tt = np.stack([rows[a] for a in keep])                      # [kept, tokens] local ids, -1 dead
    if len(keep) < n:
        remap = np.full(n + 1, -1, np.int16)                    # (remap[-1] = -1)
        remap[keep] = np.arange(len(keep), dtype=np.int16)
        tt = remap[tt]
    acc = acc[keep]
    S = len(keep) + 1
    if S > max_states:
        raise ValueError(f"grammar needs {S} states, more than {max_states}")
    dead = np.nonzero(~acc & ~(tt >= 0).any(1))[0]
    if dead.size:
        raise ValueError(f"grammar state {int(dead[0])} allows no token of this vocabulary")
    nxt = np.full((S, V), -1, np.int16)
    nxt[:S - 1, ids] = tt
    sink = S - 1
    for s in np.nonzero(acc)[0].tolist():
        nxt[s, eos] = sink
    nxt[sink, eos] = sink
    return Grammar(nxt, key)


def compile(spec: dict, tok_bytes, eos_ids, max_states: int = MAX_STATES) -> Grammar:  # noqa: A001
    """``spec`` ({"choice": [...]} | {"regex": "..."} | {"json_schema": {...}}) -> Grammar."""
    key = spec_key(spec)
    return compile_dfa(regex_to_dfa(spec_to_regex(spec)), tok_bytes, eos_ids, max_states, key)


# ------------------------------------------------------------------ kernel contracts --
def _t(a, dtype):
    import torch

    return a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a), dtype=dtype)


def mask_reference(logits, next, base, state, rows=None):  # noqa: A002
    """``ops.grammar_mask`` in plain torch, in place on fp32 ``logits`` [n, V]: row i with
    base[i] >= 0 gets -inf wherever next[base[i] + state[rows[i]], v] < 0; every other entry, and
    every row with base[i] < 0, is untouched.  ``rows`` defaults to 0..n-1."""
    import torch

    assert logits.dtype == torch.float32
    n, V = logits.shape
    nx, base, state = _t(next, torch.int16), _t(base, torch.int32), _t(state, torch.int32)
    rows = torch.arange(n) if rows is None else _t(rows, torch.int32)
    for i in range(n):
        b = int(base[i])
        if b < 0:
            continue
        bad = nx[b + int(state[int(rows[i])]), :V].to(logits.device) < 0
        logits[i][bad] = float("-inf")
    return logits


def advance_reference(next, base, state, tok, rows=None, vocab=None):  # noqa: A002
    """``ops.grammar_advance`` in plain torch, in place on ``state``: row i with base[i] >= 0 reads
    nx = next[base[i] + state[rows[i]], clamp(tok[i], 0, V - 1)] and stores it when nx >= 0.
    ``vocab``: V when ``next`` is an arena with padded rows (default: its row length)."""
    import torch

    nx, base = _t(next, torch.int16), _t(base, torch.int32)
    tok = _t(tok, torch.int64)
    n = tok.numel()
    rows = torch.arange(n) if rows is None else _t(rows, torch.int32)
    V = nx.shape[1] if vocab is None else int(vocab)
    for i in range(n):
        b = int(base[i])
        if b < 0:
            continue
        r = int(rows[i])
        v = int(nx[b + int(state[r]), min(max(int(tok[i]), 0), V - 1)])
        if v >= 0:
            state[r] = v
    return state
