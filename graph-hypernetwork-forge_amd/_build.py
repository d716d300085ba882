"""Compile csrc/*.hip for gfx950 into libghf_hip.so, in-tree (hipcc cross-compiles without a GPU)."""

from __future__ import annotations

import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor
from typing import List

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
OBJ_DIR = os.path.join(CSRC, "_obj")
LIB_PATH = os.path.join(PKG_DIR, "libghf_hip.so")
INCLUDE = os.path.join(os.path.dirname(PKG_DIR), "include")

SOURCES = ["capi.hip", "plan.hip", "text_encoder.hip", "score.hip", "backward.hip", "weightgen.hip", "weightgen_bwd.hip", "input_proj.hip", "message_generic.hip", "message_pp.hip", "message_bx.hip", "message_rs.hip", "exchange.hip", "subgraph.hip", "rank.hip", "softmax.hip", "bce.hip", "negsamp.hip", "negatives.hip", "distance.hip", "pairwise.hip", "distance_sweep.hip", "distance_loss.hip", "pairwise_sweep.hip", "pairwise_dot_sweep.hip", "candidates.hip", "relation.hip", "relation_predict.hip"]
HEADERS = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join(INCLUDE, "ghf.h"), os.path.join(INCLUDE, "ghf_negatives.h"), os.path.join(INCLUDE, "ghf_distance.h"), os.path.join(INCLUDE, "ghf_distance_sweep.h"), os.path.join(INCLUDE, "ghf_distance_loss.h"), os.path.join(INCLUDE, "ghf_pairwise.h"), os.path.join(INCLUDE, "ghf_pairwise_sweep.h"), os.path.join(INCLUDE, "ghf_pairwise_dot_sweep.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wno-unused-result"]


def hipcc_path() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: cannot build libghf_hip.so")


def _stale(target: str, deps: List[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    """Build (if stale) and return the path of libghf_hip.so."""
    hipcc = hipcc_path()
    os.makedirs(OBJ_DIR, exist_ok=True)
    jobs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ_DIR, src.replace(".hip", ".o"))
        if force or _stale(o, [s] + HEADERS):
            jobs.append((s, o))

    def compile_one(job):
        s, o = job
        cmd = [hipcc] + FLAGS + ["-c", s, "-o", o]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {s}:\n{r.stdout}\n{r.stderr}")
        return o

    if jobs:
        with ThreadPoolExecutor(max_workers=min(6, len(jobs))) as ex:
            list(ex.map(compile_one, jobs))
    objs = [os.path.join(OBJ_DIR, s.replace(".hip", ".o")) for s in SOURCES]
    if force or jobs or _stale(LIB_PATH, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    return LIB_PATH


if __name__ == "__main__":
    print(build(verbose=True))
