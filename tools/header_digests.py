#!/usr/bin/env python3
"""SHA-256 of everything the code generator derives from a traced program, over a corpus with heavy columns, sequential
sums and multi-phase defect groups: ``emit_header`` ("LimitError" where ``check_limits`` refuses the program),
``sparsity`` (both arrays' bytes) and ``sorted(lds_window(P).items())``.  A change of ``codegen.py`` that is meant to
leave the generated text alone is checked by running this before and after (also under ``OG_FUSED_COLS=4``,
``OG_FUSED_COLS=8`` and ``OG_TILE_COLS=3``) and comparing the outputs; nothing is recorded, so that an intended change
of the generator stays possible.  usage: tools/header_digests.py > digests.txt"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from opengoddard_amd import build, codegen, problems     # noqa: E402

build.build_core()
import test_edge_problems as edge        # noqa: E402
import test_module_limits as limits      # noqa: E402
import test_random_layouts as layouts    # noqa: E402


def sha(*chunks):
    h = hashlib.sha256()
    for c in chunks:
        h.update(c if isinstance(c, bytes) else str(c).encode())
    return h.hexdigest()


def corpus():
    for name in problems.NAMES:
        yield name, lambda name=name: problems.build(name)
    for name in sorted(edge.CASES):
        yield "edge:" + name, edge.CASES[name]
    for seed, shape in layouts.CASES:
        yield "layout:%d" % seed, lambda seed=seed, shape=shape: layouts.make_problem(shape, seed)
    for key in limits.SHAPES:
        yield "limit:" + key, lambda key=key: limits.problem(key)
    yield "limit:over_the_evaluation_lds", lambda: layouts.make_problem(*limits.OVER_THE_EVALUATION_LDS)


for name, make in corpus():
    P = codegen.trace_problem(*make())
    try:
        header = sha(codegen.emit_header(P))
    except codegen.LimitError:
        header = "LimitError"
    indptr, rows = codegen.sparsity(P)
    print(name, header, sha(indptr.tobytes(), rows.tobytes()), sha(sorted(codegen.lds_window(P).items())))
