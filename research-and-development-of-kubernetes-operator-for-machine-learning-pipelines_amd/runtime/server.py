"""The predictor container: V2 ("kfserving") inference protocol server (G6).

Endpoints (the SeldonDeployment's ``protocol: kfserving`` / Open Inference Protocol):
  GET  /v2/health/live | /v2/health/ready | /v2 | /v2/models/{m} | /v2/models/{m}/ready
  POST /v2/models/{m}/infer             tensors in / tensors out (sklearn or LLM)
  POST /v2/models/{m}/generate          {"text_input" | "input_ids", "parameters": {...}}
  POST /v2/models/{m}/generate_stream   server-sent events, one per token
  POST /api/v1.0/feedback               Seldon feedback (counted as service="feedback")
  GET  /metrics                         Prometheus exposition (runtime/metrics.py)

Every request is timed into the Seldon-executor histograms with its HTTP
code, which is what the operator's canary gate queries.

``python -m mlopamd.runtime.server --runtime mlop-llm --architecture llama3-8b``
starts it; configuration also comes from the env the SeldonDeployment sets
(MLOP_RUNTIME, MLOP_MODEL_URI, MLOP_ARCHITECTURE, MLOP_ENGINE_*, MLOP_DTYPE).  A model URI that
resolves to a local Hugging Face checkpoint (models/loader.py) is served with its weights and
``tokenizer.json``; otherwise the architecture is random-initialised (the benchmark setup).
Fault injection for canary tests: MLOP_INJECT_LATENCY_S, MLOP_INJECT_ERROR_RATE,
MLOP_INJECT_START_ERROR (fail at start-up, e.g. a GPU OOM message), MLOP_INJECT_CRASH_AFTER_S
(exit with status 139 after serving that long).
"""
from __future__ import annotations

import argparse
import asyncio
import json
import os
import random
import time

import numpy as np

# start-up phases of this predictor process, seconds since the OS created it (GET /v2/debug/startup;
# bench.py's fresh-process CR -> ready probe reports them): what the 2 s of a cold start go to
STARTUP: dict = {}


def _since_process_start() -> float:
    """Seconds since the launcher started this process (MLOP_LAUNCH_EPOCH, its wall clock right
    before the spawn: exact on one host), else since the kernel's process creation time (psutil:
    clock-tick resolution on an integer-second boot time, so only differences are meaningful)."""
    t0 = os.environ.get("MLOP_LAUNCH_EPOCH")
    if t0:
        return round(time.time() - float(t0), 3)
    try:
        import psutil

        return round(time.time() - psutil.Process().create_time(), 3)
    except Exception:  # noqa: BLE001
        return -1.0


STARTUP["server_module_imported_s"] = _since_process_start()
if os.environ.get("MLOP_LAUNCHER_INFO"):  # this rank's pod launcher (rank_launcher.py) about itself
    STARTUP["launcher"] = json.loads(os.environ["MLOP_LAUNCHER_INFO"])

if __name__ == "__main__":
    import sys as _sys

    # one module object whether reached as __main__ or as a package import (tp_worker /
    # ep_serving import make_app from here): one STARTUP dict, one set of globals
    _sys.modules.setdefault(f"{__package__}.server", _sys.modules[__name__])

    # a multi-rank pod's container process is a LAUNCHER: decided from argv / env alone, before
    # torch is imported and before any HIP call, and it never comes back here (rank_launcher.py)
    from .rank_launcher import launch_ranks as _launch_ranks, launcher_degree as _launcher_degree

    _n_ranks = _launcher_degree(_sys.argv[1:])
    if _n_ranks > 1:
        raise SystemExit(_launch_ranks(_n_ranks, _sys.argv[1:]))


def _warm_hip() -> None:
    """Initialise the HIP runtime and this rank's device context on a helper thread WHILE torch
    imports (~1.4 s of Python and dlopen): the C calls release the GIL, and torch's own first
    device call then finds the runtime up (first allocation 0.15-0.35 s -> ~0.1 s,
    scripts/probe_startup.py).  Off for CPU predictors and with MLOP_HIP_WARMUP=0."""
    import ctypes
    import importlib.util

    try:
        # torch's OWN copy of the runtime (its lib/ directory, found without importing torch): a
        # bare "libamdhip64.so" could resolve to the system ROCm copy, and a second HIP runtime
        # in the process would not be the one torch and _C.so launch on
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        lib = ctypes.CDLL(os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so"))
        if lib.hipInit(0) == 0 and lib.hipSetDevice(int(os.environ.get("LOCAL_RANK", "0"))) == 0:
            lib.hipFree(ctypes.c_void_p(0))  # creates the device context
        STARTUP["hip_warm_s"] = _since_process_start()
    except OSError:
        pass


def start_hip_warmup() -> bool:
    """Start ``_warm_hip`` on a daemon thread in a process that will itself run a GPU engine:
    the predictor's ``__main__`` once it is known not to be a multi-rank launcher (above), never
    on import as a library.  Off for CPU / sklearn predictors and with MLOP_HIP_WARMUP=0."""
    if (os.environ.get("MLOP_DEVICE", "cuda") == "cpu" or os.environ.get("MLOP_HIP_WARMUP", "1") == "0"
            or os.environ.get("MLOP_RUNTIME", "mlop-llm") in ("mlop-sklearn", "sklearn")):
        return False
    import threading

    from . import rank_launcher

    rank_launcher.WARMUP_STARTED = True
    STARTUP["hip_warmup_started"] = True
    threading.Thread(target=_warm_hip, name="hip-warmup", daemon=True).start()
    return True


if __name__ == "__main__":
    start_hip_warmup()

from .sampler import SamplingParams  # noqa: E402 (imports torch: timed below)

STARTUP["torch_imported_s"] = _since_process_start()

_DT = {"FP32": np.float32, "FP64": np.float64, "INT64": np.int64, "INT32": np.int32, "FP16": np.float16,
       "BOOL": np.bool_, "UINT8": np.uint8}
_DT_NAME = {np.dtype(v): k for k, v in _DT.items()}


def _params(p: dict) -> SamplingParams:
    lp = p.get("logprobs")
    if lp is not None and (isinstance(lp, bool) or not isinstance(lp, int)):
        raise ValueError(f"logprobs must be an int, got {lp!r}")
    ad = p.get("adapter")
    if ad is not None and not isinstance(ad, str):
        raise ValueError(f"adapter must be a string, got {ad!r}")
    # guided decoding: at most one of guided_choice / guided_regex / guided_json
    given = [k for k in ("guided_choice", "guided_regex", "guided_json") if p.get(k) is not None]
    if len(given) > 1:
        raise ValueError(f"at most one of guided_choice / guided_regex / guided_json, got {given}")
    guided = None
    if given:
        v = p[given[0]]
        if given[0] == "guided_choice":
            if not isinstance(v, list) or not v or any(not isinstance(c, str) for c in v):
                raise ValueError("guided_choice must be a non-empty list of strings")
            guided = {"choice": v}
        elif given[0] == "guided_regex":
            if not isinstance(v, str):
                raise ValueError(f"guided_regex must be a string, got {type(v).__name__}")
            guided = {"regex": v}
        else:
            if isinstance(v, str):
                try:
                    v = json.loads(v)
                except ValueError as e:
                    raise ValueError(f"guided_json is not valid JSON: {e}") from None
            if not isinstance(v, dict):
                raise ValueError("guided_json must be a JSON schema object (or its JSON text)")
            guided = {"json_schema": v}
    pooling = p.get("pooling")
    if pooling is not None and not isinstance(pooling, str):
        raise ValueError(f"pooling must be a string, got {pooling!r}")
    if pooling is None and (p.get("normalize") is not None or p.get("dimensions") is not None):
        raise ValueError("normalize / dimensions need pooling (an embedding request)")
    emb = {}
    if pooling is not None:
        norm, dim = p.get("normalize", True), p.get("dimensions")
        if not isinstance(norm, bool):
            raise ValueError(f"normalize must be a bool, got {norm!r}")
        if dim is not None and (isinstance(dim, bool) or not isinstance(dim, int)):
            raise ValueError(f"dimensions must be an int, got {dim!r}")
        if p.get("encoding_format") not in (None, "float"):
            raise ValueError("only float (JSON number) embeddings are served: no base64 / fp16 encodings")
        emb = {"embed": pooling, "embed_normalize": norm, "embed_dim": dim}
    return SamplingParams(**emb, adapter=ad, guided=guided,max_tokens=int(p.get("max_tokens", 64)), temperature=float(p.get("temperature", 0.0)),
                          top_k=int(p.get("top_k", 0)), top_p=float(p.get("top_p", 1.0)),
                          ignore_eos=bool(p.get("ignore_eos", False)),
                          stop_token_ids=list(p.get("stop_token_ids", [])),
                          seed=None if p.get("seed") is None else int(p["seed"]),
                          repetition_penalty=float(p.get("repetition_penalty", 1.0)),
                          presence_penalty=float(p.get("presence_penalty", 0.0)),
                          frequency_penalty=float(p.get("frequency_penalty", 0.0)),
                          logprobs=lp).validate()


def _logprob_outputs(res: dict, n: int) -> list:
    """V2 output tensors of a request's log-probabilities: ``logprobs`` FP32 [T] and, for n > 0,
    ``top_logprob_ids`` INT64 [T, n] / ``top_logprobs`` FP32 [T, n]."""
    lps = res["logprobs"]
    T = len(lps)
    outs = [{"name": "logprobs", "shape": [T], "datatype": "FP32", "data": [e["logprob"] for e in lps]}]
    if n > 0:
        outs.append({"name": "top_logprob_ids", "shape": [T, n], "datatype": "INT64",
                     "data": [t[0] for e in lps for t in e["top"]]})
        outs.append({"name": "top_logprobs", "shape": [T, n], "datatype": "FP32",
                     "data": [t[1] for e in lps for t in e["top"]]})
    return outs


def make_app(backend, metrics, version: str = "1", inject_latency_s: float | None = None,
             inject_error_rate: float | None = None):
    from aiohttp import web

    lat = float(os.environ.get("MLOP_INJECT_LATENCY_S", inject_latency_s or 0.0))
    err_rate = float(os.environ.get("MLOP_INJECT_ERROR_RATE", inject_error_rate or 0.0))
    state = {"ready": getattr(backend, "ready", True)}

    @web.middleware
    async def timing(request, handler):
        t0 = time.perf_counter()
        service = "feedback" if request.path.endswith("/feedback") else (
            "generate" if "generate" in request.path else "predictions")
        code = 500
        try:
            if request.method == "POST" and not request.path.endswith("/feedback"):
                if lat:
                    await asyncio.sleep(lat)
                if err_rate and random.random() < err_rate:
                    raise web.HTTPInternalServerError(text="injected failure")
            try:
                resp = await handler(request)
            except ValueError as e:  # a request the engine refuses (engine.check_request): the client's error
                raise web.HTTPBadRequest(text=str(e)) from None
            code = resp.status
            return resp
        except web.HTTPException as e:
            code = e.status
            raise
        finally:
            if request.method == "POST" and metrics is not None:
                metrics.observe_request(time.perf_counter() - t0, code=code, service=service)

    app = web.Application(middlewares=[timing], client_max_size=64 * 2**20)

    def req_params(p: dict) -> SamplingParams:
        """Parsed and validated sampling parameters (ValueError -> 400), including what this
        backend cannot serve (an expert-parallel predictor: no log-probabilities)."""
        params = _params(p)
        check = getattr(backend, "check_params", None)
        if check is not None:
            check(params)
        return params

    def gen_params(p: dict) -> SamplingParams:
        """``req_params`` of a request that generates tokens: embedding parameters are refused (400),
        they belong to /embed or to infer's embedding form."""
        params = req_params(p)
        if params.embed is not None:
            raise ValueError("parameters.pooling asks for an embedding: use POST /v2/models/{m}/embed or infer, "
                             "not a generation endpoint")
        return params

    async def live(_):
        return web.json_response({"live": True})

    async def ready(_):
        ok = bool(getattr(backend, "ready", True))
        return web.json_response({"ready": ok}, status=200 if ok else 503)

    async def server_meta(_):
        return web.json_response({"name": "mlopamd-runtime", "version": "0.1.0",
                                  "extensions": ["generate", "metrics"]})

    async def model_meta(req):
        md = backend.metadata()
        md["versions"] = [version]
        return web.json_response(md)

    async def infer(req):
        body = await req.json()
        inputs = {i["name"]: i for i in body.get("inputs", [])}
        if backend.kind == "sklearn":
            first = next(iter(inputs.values()))
            x = np.asarray(first["data"], dtype=_DT.get(first.get("datatype", "FP32"), np.float32))
            x = x.reshape(first.get("shape", x.shape))
            y = backend.predict(x)
            y = np.asarray(y)
            dt = _DT_NAME.get(y.dtype, "BYTES")
            data = y.tolist() if dt != "BYTES" else [str(v) for v in y.tolist()]
            return web.json_response({"model_name": backend.name, "model_version": version,
                                      "id": body.get("id", ""), "outputs": [
                                          {"name": "predict", "shape": list(y.shape), "datatype": dt, "data": data}]})
        if (body.get("parameters") or {}).get("pooling") is not None or getattr(backend, "embedding_only", False):
            # an embedding request: n strings, or one input_ids tensor -> one FP32 [n, d] tensor
            params = embed_params(body.get("parameters"))
            if "input_ids" in inputs:
                prompts = [[int(v) for v in inputs["input_ids"]["data"]]]
            else:
                prompts = [backend.tokenizer.encode(str(t)) for t in inputs["text_input"]["data"]]
            res, d, n = await run_embed(prompts, params)
            data = [float(x) for r in res for x in r["embedding"]]
            return web.json_response({"model_name": backend.name, "model_version": version, "id": body.get("id", ""),
                                      "outputs": [{"name": "embedding", "shape": [len(res), d], "datatype": "FP32",
                                                   "data": data}],
                                      "parameters": {"prompt_tokens": n}})
        params = gen_params(body.get("parameters", {}))
        if "input_ids" in inputs:
            ids = [int(v) for v in inputs["input_ids"]["data"]]
            res = await backend.generate(ids, params)
            out = {"name": "output_ids", "shape": [len(res["output_ids"])], "datatype": "INT64",
                   "data": res["output_ids"]}
        else:
            text = inputs["text_input"]["data"][0]
            res = await backend.generate(backend.tokenizer.encode(text), params)
            out = {"name": "text_output", "shape": [1], "datatype": "BYTES",
                   "data": [backend.tokenizer.decode(res["output_ids"])]}
        outs = [out]
        if params.logprobs is not None:
            outs += _logprob_outputs(res, params.logprobs)
        return web.json_response({"model_name": backend.name, "model_version": version, "id": body.get("id", ""),
                                  "outputs": outs, "parameters": {"finish_reason": res["finish_reason"]}})

    def embed_params(p: dict) -> SamplingParams:
        """An embedding request's parameters: pooling / normalize default to the checkpoint's own
        settings (sentence-transformers files; last, normalised without them)."""
        p = dict(p or {})
        pooling, normalize = backend.embedding_defaults() if hasattr(backend, "embedding_defaults") else (None, True)
        if p.get("pooling") is None:
            if pooling is None:
                raise ValueError("this checkpoint names no pooling mode this runtime serves: the request must set "
                                 "parameters.pooling (last | mean)")
            p["pooling"] = pooling
        if p.get("normalize") is None:  # (whether or not the request names its pooling)
            p["normalize"] = normalize
        return req_params(p)

    async def run_embed(prompts, params):
        """-> (results, d, prompt tokens); every input is checked before any is queued (400, none runs)."""
        if not prompts:
            raise ValueError("no input to embed")
        check = getattr(getattr(backend, "engine", None), "check_request", None)
        for ids in prompts:
            if check is not None:
                check(ids, params)  # empty / longer than max_model_len (never truncated) / ids outside the vocabulary
        res = await backend.embed(prompts, params)
        return res, int(res[0]["embedding"].shape[0]), sum(r["prompt_tokens"] for r in res)

    def id_lists(v) -> list:
        if not isinstance(v, list) or not v:
            raise ValueError("input_ids must be a non-empty list of ints or of such lists")
        rows = v if isinstance(v[0], list) else [v]
        if any(not isinstance(r, list) or any(isinstance(t, bool) or not isinstance(t, int) for t in r) for r in rows):
            raise ValueError("input_ids must be a non-empty list of ints or of such lists")
        return rows

    async def embed(req):
        if backend.kind != "llm":
            raise web.HTTPBadRequest(text="embed is only served by LLM predictors")
        body = await req.json()
        params = embed_params(body.get("parameters"))
        if "input_ids" in body:
            prompts = id_lists(body["input_ids"])
        else:
            texts = body.get("text_input")
            texts = [texts] if isinstance(texts, str) else texts
            if not isinstance(texts, list) or not texts or any(not isinstance(t, str) for t in texts):
                raise ValueError("text_input must be a string or a non-empty list of strings")
            prompts = [backend.tokenizer.encode(t) for t in texts]
        res, d, n = await run_embed(prompts, params)
        return web.json_response({"model_name": backend.name, "model_version": version,
                                  "embeddings": [r["embedding"].tolist() for r in res], "dimensions": d,
                                  "usage": {"prompt_tokens": n}})

    async def generate(req):
        if backend.kind != "llm":
            raise web.HTTPBadRequest(text="generate is only served by LLM predictors")
        body = await req.json()
        params = gen_params(body.get("parameters", body))
        ids = body["input_ids"] if "input_ids" in body else backend.tokenizer.encode(body.get("text_input", ""))
        res = await backend.generate(ids, params)
        out = {"model_name": backend.name, "model_version": version,
               "text_output": backend.tokenizer.decode(res["output_ids"]),
               "output_ids": res["output_ids"], "finish_reason": res["finish_reason"],
               "usage": {"prompt_tokens": res["prompt_tokens"], "completion_tokens": len(res["output_ids"])},
               "ttft_s": res["ttft"], "latency_s": res["latency"]}
        if params.logprobs is not None:  # one entry per completion token
            out["logprobs"] = res["logprobs"]
        return web.json_response(out)

    async def generate_stream(req):
        if backend.kind != "llm":
            raise web.HTTPBadRequest(text="generate_stream is only served by LLM predictors")
        body = await req.json()
        params = gen_params(body.get("parameters", body))
        ids = body["input_ids"] if "input_ids" in body else backend.tokenizer.encode(body.get("text_input", ""))
        r = backend.submit(ids, params, stream=True)
        resp = web.StreamResponse(headers={"Content-Type": "text/event-stream"})
        await resp.prepare(req)
        while True:
            tok = await r.queue.get()
            if tok is None:
                break
            extra = {}
            if isinstance(tok, tuple):  # (token, logprob, top): the request asked for log-probabilities
                tok, lp, top = tok
                extra = {"logprob": lp, "top_logprobs": [list(t) for t in top]}
            ev = {"token_id": tok, "text_output": backend.tokenizer.decode([tok]), **extra}
            await resp.write(f"data: {json.dumps(ev)}\n\n".encode())
        res = await r.future
        await resp.write(f"data: {json.dumps({'finish_reason': res['finish_reason'], 'done': True})}\n\n".encode())
        await resp.write_eof()
        return resp

    async def trace(_):
        eng = getattr(backend, "engine", None)
        if eng is None or not hasattr(eng, "tracer"):
            raise web.HTTPNotFound(text="no engine tracer on this predictor")
        return web.json_response(eng.tracer.chrome_trace())

    async def trace_summary(_):
        eng = getattr(backend, "engine", None)
        if eng is None or not hasattr(eng, "tracer"):
            raise web.HTTPNotFound(text="no engine tracer on this predictor")
        return web.json_response({"steps": eng.tracer.summary(), "stats": dict(eng.stats)})

    async def feedback(req):
        await req.read()
        return web.json_response({"status": "ok"})

    async def prom(_):
        if metrics is None:
            return web.Response(text="")
        try:
            from .gpu_metrics import sample

            metrics.update_gpu(sample())
        except Exception:  # noqa: BLE001
            pass
        return web.Response(body=metrics.exposition(), content_type="text/plain", charset="utf-8")

    r = app.router
    r.add_get("/v2/health/live", live)
    r.add_get("/v2/health/ready", ready)
    r.add_get("/v2", server_meta)
    r.add_get("/v2/models/{m}", model_meta)
    r.add_get("/v2/models/{m}/ready", ready)
    r.add_post("/v2/models/{m}/infer", infer)
    r.add_post("/v2/models/{m}/generate", generate)
    r.add_post("/v2/models/{m}/embed", embed)
    r.add_post("/v2/models/{m}/generate_stream", generate_stream)
    r.add_post("/api/v1.0/feedback", feedback)
    r.add_post("/api/v1.0/predictions", infer)
    r.add_get("/metrics", prom)
    r.add_get("/v2/debug/trace", trace)            # Chrome / Perfetto trace of recent engine steps
    r.add_get("/v2/debug/steps", trace_summary)

    async def startup(_):
        return web.json_response(STARTUP)

    async def on_start(_app):
        STARTUP["http_listening_s"] = _since_process_start()

    r.add_get("/v2/debug/startup", startup)
    app.on_startup.append(on_start)
    return app


def build_backend(runtime: str, model_uri: str | None, architecture: str | None, name: str, metrics,
                  device: str = "cuda", engine_kwargs: dict | None = None, seed: int = 0, tp_state=None):
    if runtime in ("mlop-sklearn", "sklearn"):
        from .backends import SklearnBackend

        return SklearnBackend(model_uri, name=name)
    from .backends import LLMBackend
    from .deploy import build_engine

    from .backends import load_tokenizer

    import torch

    t0 = time.perf_counter()
    STARTUP["engine_build_start_s"] = _since_process_start()
    dtype = {"float32": torch.float32, "bfloat16": torch.bfloat16}[os.environ.get("MLOP_DTYPE", "bfloat16")]
    eng = build_engine(architecture or "llama3-8b", device=device, seed=seed, tp_state=tp_state,
                       model_uri=model_uri, dtype=dtype, **(engine_kwargs or {}))
    load_env_adapters(eng)
    STARTUP["engine_built_s"] = _since_process_start()
    STARTUP["engine"] = {k: int(eng.stats.get(k, 0)) for k in ("model_build_ms", "kv_alloc_ms", "graph_capture_ms")}
    from .. import ops

    # serving must never time GEMM candidates mid-request (a canary's latency would spike on
    # every first-seen batch size): decide from the shipped table / nearest tuned row count
    ops.freeze_autotune()
    if metrics is not None:
        metrics.load_seconds.labels(**metrics.labels).set(time.perf_counter() - t0)
        metrics.ready.labels(**metrics.labels).set(1)
    return LLMBackend(eng, metrics, tokenizer=load_tokenizer(eng.checkpoint_dir), name=name).start()


def load_env_adapters(eng) -> list:
    """Load the LoRA adapters of ``MLOP_ADAPTERS`` (JSON ``[{"name": ..., "uri": ...}]``, set by the
    operator from ``spec.adapters``) before the predictor reports ready.  URIs follow the model
    URI rules (``models.loader.resolve_adapter_dir``); one that does not resolve fails start-up."""
    raw = os.environ.get("MLOP_ADAPTERS")
    if not raw:
        return []
    from ..models.loader import resolve_adapter_dir

    specs = json.loads(raw)
    if not isinstance(specs, list) or not all(isinstance(a, dict) and a.get("name") and a.get("uri") for a in specs):
        raise ValueError("MLOP_ADAPTERS must be a JSON list of {\"name\": ..., \"uri\": ...}")
    for a in specs:
        d = resolve_adapter_dir(a["uri"])
        if d is None:
            raise FileNotFoundError(f"adapter {a['name']!r}: no adapter_config.json reachable at {a['uri']!r}")
        eng.load_adapter(a["name"], d)
    return [a["name"] for a in specs]


def engine_kwargs_from_env() -> dict:
    out = {}
    for k, v in os.environ.items():
        if k.startswith("MLOP_ENGINE_"):
            key = k[len("MLOP_ENGINE_"):].lower()
            try:
                out[key] = json.loads(v)
            except ValueError:
                out[key] = v
    return out


def main(argv=None):
    import sys

    argv = list(sys.argv[1:] if argv is None else argv)
    ap = argparse.ArgumentParser(description="mlopamd V2 inference server")
    ap.add_argument("--host", default="0.0.0.0")
    ap.add_argument("--port", type=int, default=int(os.environ.get("MLOP_PORT", 9000)))
    ap.add_argument("--runtime", default=os.environ.get("MLOP_RUNTIME", "mlop-llm"))
    ap.add_argument("--model-uri", default=os.environ.get("MLOP_MODEL_URI"))
    ap.add_argument("--architecture", default=os.environ.get("MLOP_ARCHITECTURE"))
    ap.add_argument("--name", default=os.environ.get("MLOP_MODEL_NAME", "model"))
    ap.add_argument("--version", default=os.environ.get("MLOP_MODEL_VERSION", "1"))
    ap.add_argument("--device", default=os.environ.get("MLOP_DEVICE", "cuda"))
    ap.add_argument("--tp", type=int, default=1)
    ap.add_argument("--ep", type=int, default=1,
                    help="expert-parallel degree with data-parallel attention (MoE; --tp 1): one "
                         "engine per GPU behind this endpoint (runtime/ep_serving.py)")
    ap.add_argument("--share-gpu", action="store_true",
                    help="one-GPU rehearsal of a --tp / --ep pod: every rank on device 0 over a gloo "
                         "group with the IPC all-reduce / exchange kernels forced (also MLOP_SHARE_GPU=1)")
    a = ap.parse_args(argv)
    if a.tp > 1 and a.ep > 1:
        raise SystemExit("--tp and --ep > 1 together: TP shards experts itself (EP = TP); use one")
    from .rank_launcher import launch_ranks, launcher_degree, share_gpu_requested

    a.share_gpu = share_gpu_requested(argv)
    n = launcher_degree(argv)
    if n > 1:  # main() called in-process (the __main__ path decided this before importing torch)
        raise SystemExit(launch_ranks(n, argv, a.share_gpu))

    from aiohttp import web

    from .metrics import RuntimeMetrics

    metrics = RuntimeMetrics(model_name=a.name)
    tp_state = None
    if a.ep > 1:
        from .ep_serving import serve_ep

        return serve_ep(a, metrics)
    if a.tp > 1 or int(os.environ.get("WORLD_SIZE", 1)) > 1:
        from .tp_worker import serve_tp

        return serve_tp(a, metrics)
    if os.environ.get("MLOP_INJECT_START_ERROR"):  # fault injection: e.g. a GPU OOM at weight load
        raise RuntimeError(os.environ["MLOP_INJECT_START_ERROR"])
    backend = build_backend(a.runtime, a.model_uri, a.architecture, a.name, metrics, a.device,
                            engine_kwargs_from_env(), tp_state=tp_state)
    crash_after = float(os.environ.get("MLOP_INJECT_CRASH_AFTER_S", 0) or 0)
    if crash_after > 0:  # fault injection: the process dies (SIGSEGV-like exit) after serving a while
        import threading

        threading.Timer(crash_after, lambda: os._exit(139)).start()
    web.run_app(make_app(backend, metrics, version=a.version), host=a.host, port=a.port, print=None)


if __name__ == "__main__":
    main()
