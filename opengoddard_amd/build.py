"""Compile the HIP sources of this package for gfx950 (in-tree, no JIT cache elsewhere).

Two artefacts:

* ``lib/libogpsx.so`` - the generic runtime and public C ABI (``include/ogpsx.h``), from
  ``csrc/ogpsx_core.hip``.
* ``lib/jit/libogk_<hash>.so`` - one callback module per traced problem: the hand-written
  sweep kernels ``csrc/ogk_kernels.hip`` instantiated with the generated device functions of
  that problem (``codegen.emit_header``).  Keyed by a hash of the generated source, so a
  problem is compiled once and the shared object travels with the tree.

``-ffp-contract=off`` is part of the numerical contract (bit parity with the CPU oracle,
SURVEY.md section 7.4 item 2); fused multiply-adds only happen where the code asks for them.
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
JITDIR = os.path.join(LIBDIR, "jit")
CORE_LIB = os.path.join(LIBDIR, "libogpsx.so")
ARCH = "gfx950"
HIP_FLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
             "-Wno-unused-value"] + os.environ.get("OG_EXTRA_HIPFLAGS", "").split()


# flags for the callback modules only (a stamped build of one workload's kernels - -DOGK_TRACE=1 - must not change the
# digest of libogpsx.so / libogsqp.so and make every later process rebuild them)
MODULE_FLAGS = os.environ.get("OG_MODULE_HIPFLAGS", "").split()


class BuildError(RuntimeError):
    pass


def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise BuildError("hipcc not found: the HIP extension cannot be built on this machine")
    return exe


def _run(cmd):
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if proc.returncode != 0:
        raise BuildError("command failed: %s\n%s" % (" ".join(cmd), proc.stdout[-4000:]))
    return proc.stdout


def _digest_files(paths, extra=""):
    """Content hash of the sources an artefact is built from (mtimes do not survive the
    snapshot copy to the GPU box, content does)."""
    hsh = hashlib.sha256(extra.encode())
    for path in paths:
        with open(path, "rb") as fh:
            hsh.update(fh.read())
    hsh.update(" ".join(HIP_FLAGS).encode())
    return hsh.hexdigest()[:16]


def _core_sources():
    return [os.path.join(CSRC, f) for f in ("ogpsx_core.hip", "og_lgl.h", "og_math.h", "ogk.h")] + \
        [os.path.join(HERE, "..", "include", "ogpsx.h")]


def _kernel_sources():
    return [os.path.join(CSRC, f) for f in ("ogk_kernels.hip", "ogk_fused_workgroup.inc", "ogk.h", "og_math.h", "og_dual.h", "og_par.h",
                                               "og_dir.h", "og_adj.h", "og_dual2.h", "og_hvp.h", "og_mix.h", "og_hess.h", "og_pp.h")]


def _build_library(lib, sources, override, force):
    """One of the two fixed libraries, from ``sources[0]`` and the headers after it -> its path.  Rebuilt when the
    content of the sources or the flags change (a stamp file next to it holds their digest).  ``override``: the
    environment variable that names a build made elsewhere, with other flags, to use instead (diagnostics)."""
    if os.environ.get(override):
        return os.environ[override]
    os.makedirs(LIBDIR, exist_ok=True)
    stamp_path = lib + ".stamp"
    want = _digest_files(sources)
    if not force and os.path.exists(lib) and os.path.exists(stamp_path):
        with open(stamp_path) as fh:
            if fh.read().strip() == want:
                return lib
    tmp = lib + ".tmp%d" % os.getpid()
    _run([hipcc()] + HIP_FLAGS + [sources[0], "-o", tmp, "-ldl"])
    os.replace(tmp, lib)
    with open(stamp_path, "w") as fh:
        fh.write(want)
    return lib


def build_core(force=False):
    """``lib/libogpsx.so`` (``OG_CORE_LIB``: tools/sanitize.sh)."""
    return _build_library(CORE_LIB, _core_sources(), "OG_CORE_LIB", force)


SQP_LIB = os.path.join(LIBDIR, "libogsqp.so")


def build_sqp(force=False):
    """``lib/libogsqp.so``: the QP subproblem / BFGS kernels of the SQP driver (``include/ogsqp.h``; ``OG_SQP_LIB``:
    a build with -DOGSQP_TRACE)."""
    sources = [os.path.join(CSRC, f) for f in ("ogsqp.hip", "ogsqp_rows.h", "ogsqp_lq16.h", "ogsqp_lqwide.h",
                                               "ogsqp_resident.h")] + [os.path.join(HERE, "..", "include", "ogsqp.h")]
    return _build_library(SQP_LIB, sources, "OG_SQP_LIB", force)


def module_digest(header_source):
    """Key of a callback module: generated header + kernel sources + flags."""
    return _digest_files(_kernel_sources(), extra=header_source + " ".join(MODULE_FLAGS))


def module_path(digest):
    return os.path.join(JITDIR, "libogk_%s.so" % digest)


# The kernel source instantiates the generated callbacks once per kernel, and code generation for them is what a
# module's build time consists of (10-15 s at C3, 40 s at C5 as one translation unit).  The kernels are therefore
# compiled as PARTS side by side (-DOGK_PART=k, csrc/ogk_kernels.hip): part 0 (evaluation, pattern, pack, unpack)
# is <module>.so, the others <module>.p<k>.so next to it; the runtime loads what is there (ogpsx_core.hip:
# ogk_module).  Wall-clock of a cold start = the slowest part.
# (csrc/ogk.h names the values: OGK_PART_MAIN, OGK_PART_FUSED, OGK_PART_SWEEP, OGK_PART_AUX)
MODULE_PARTS = (0, 2, 3, 1)     # OGK_PART of <module>.so, .p1.so, .p2.so, .p3.so: main, one-launch sweep, sweep, aux


def part_path(out, index):
    return out if index == 0 else out[:-3] + ".p%d.so" % index


BATCH_PART = 4                  # OGK_PART_BATCH, <module>.batch.so: the kernels of a batch of points (og_batch_*)


def batch_part_path(out):
    return out[:-3] + ".batch.so"


def _write_header(header_source, digest):
    """The generated header of a module, next to its shared objects (written through a temporary file: concurrent
    builds of one digest see a whole file) -> its path."""
    header = os.path.join(JITDIR, "og_gen_%s.h" % digest)
    with tempfile.NamedTemporaryFile("w", dir=JITDIR, suffix=".h", delete=False) as fh:
        fh.write(header_source)
        tmp_header = fh.name
    os.replace(tmp_header, header)
    return header


def _build_on_demand_part(header_source, part, path_of, force):
    """Compile one ``OGK_PART`` of csrc/ogk_kernels.hip that is none of ``MODULE_PARTS`` against one generated header
    -> ``path_of(<module>.so)``, next to the module of the same digest and cached like it."""
    os.makedirs(JITDIR, exist_ok=True)
    digest = module_digest(header_source)
    out = path_of(module_path(digest))
    if not force and os.path.exists(out):
        return out
    header = _write_header(header_source, digest)
    tmp = out + ".tmp%d" % os.getpid()
    _run([hipcc()] + HIP_FLAGS + MODULE_FLAGS + ["-DOGK_PART=%d" % part, "-I" + CSRC, "-DOG_GEN_HEADER=\"%s\"" % header,
                                                 os.path.join(CSRC, "ogk_kernels.hip"), "-o", tmp])
    os.replace(tmp, out)
    return out


def build_batch_part(header_source, force=False):
    """The batch kernels (``ogk_fused_batch`` / ``ogk_eval_batch``, ``OGK_PART=4``) -> path of ``<module>.batch.so``.
    Not one of ``MODULE_PARTS``: it is built when a batch is first asked for (``HipEngine.batch``), so that
    ``build_module`` and the cold start of a user who never batches stay what they are."""
    return _build_on_demand_part(header_source, BATCH_PART, batch_part_path, force)


BATCH_EXACT_PART = 5            # OGK_PART_BATCH_EXACT, <module>.batchx.so: the exact Jacobian of a batch


def batch_exact_part_path(out):
    return out[:-3] + ".batchx.so"


def build_batch_exact_part(header_source, force=False):
    """``ogk_exact_struct_batch`` (``OGK_PART=5``) -> path of ``<module>.batchx.so``.  A part of its own, neither one
    of ``MODULE_PARTS`` nor in the batch part: the kernel instantiates the callbacks on dual numbers, and a user who
    batches evaluations or FD sweeps only builds and loads what they did before.  Built when an exact Jacobian of a
    batch is first asked for (``BatchSweep.exact``)."""
    return _build_on_demand_part(header_source, BATCH_EXACT_PART, batch_exact_part_path, force)


PARAMETER_PART = 6              # OGK_PART_PAR, <module>.par.so: exact dF/dtheta for run-time parameters


def parameter_part_path(out):
    return out[:-3] + ".par.so"


def build_parameter_part(header_source, force=False):
    """``ogk_exact_par`` / ``ogk_exact_par_batch`` (``OGK_PART=6``) -> path of ``<module>.par.so``.  A part of its own,
    built when an exact parameter Jacobian is first asked for (``HipEngine.parameter_jacobian``,
    ``BatchSweep.parameter_jacobian``): the module and the two batch parts are what they were, and a user who never asks
    builds and loads what they did before."""
    return _build_on_demand_part(header_source, PARAMETER_PART, parameter_part_path, force)


DIRECTIONAL_PART = 7            # OGK_PART_DIR, <module>.dir.so: exact directional derivatives F'(x) v


def directional_part_path(out):
    return out[:-3] + ".dir.so"


def build_directional_part(header_source, force=False):
    """``ogk_exact_dir`` / ``ogk_exact_dir_batch`` (``OGK_PART=7``) -> path of ``<module>.dir.so``.  A part of its own,
    built when a directional derivative is first asked for (``HipEngine.directional``, ``BatchSweep.directional``): the
    module and the other on-demand parts are what they were, and a user who never asks builds and loads what they did
    before."""
    return _build_on_demand_part(header_source, DIRECTIONAL_PART, directional_part_path, force)


ADJOINT_PART = 8                # OGK_PART_ADJ, <module>.adj.so: exact adjoint products F'(x)^T w


def adjoint_part_path(out):
    return out[:-3] + ".adj.so"


def build_adjoint_part(header_source, force=False):
    """``ogk_exact_adj`` / ``ogk_exact_adj_batch`` (``OGK_PART=8``) -> path of ``<module>.adj.so``.  A part of its own,
    built when an adjoint product is first asked for (``HipEngine.adjoint``, ``BatchSweep.adjoint``): the module and the
    other on-demand parts are what they were, and a user who never asks builds and loads what they did before."""
    return _build_on_demand_part(header_source, ADJOINT_PART, adjoint_part_path, force)


HESSIAN_PART = 9                # OGK_PART_HVP, <module>.hvp.so: exact Hessian-vector products of w . F


def hessian_part_path(out):
    return out[:-3] + ".hvp.so"


def build_hessian_part(header_source, force=False):
    """``ogk_exact_hvp`` / ``ogk_exact_hvp_batch`` (``OGK_PART=9``) -> path of ``<module>.hvp.so``.  A part of its own,
    built when a Hessian-vector product is first asked for (``HipEngine.hessian_vector``,
    ``BatchSweep.hessian_vector``): the module and the other on-demand parts are what they were, and a user who never
    asks builds and loads what they did before."""
    return _build_on_demand_part(header_source, HESSIAN_PART, hessian_part_path, force)


MIX_PART = 10                   # OGK_PART_MIX, <module>.mix.so: exact mixed derivatives d(F'(x)^T w)/dtheta


def mix_part_path(out):
    return out[:-3] + ".mix.so"


def build_mix_part(header_source, force=False):
    """``ogk_exact_mix`` / ``ogk_exact_mix_batch`` (``OGK_PART=10``) -> path of ``<module>.mix.so``.  A part of its own,
    built when a mixed derivative is first asked for (``HipEngine.adjoint_parameter``,
    ``BatchSweep.adjoint_parameter``): the module and the other on-demand parts are what they were, and a user who never
    asks builds and loads what they did before."""
    return _build_on_demand_part(header_source, MIX_PART, mix_part_path, force)


HESSIAN_MATRIX_PART = 11        # OGK_PART_HESS, <module>.hess.so: the exact sparse Hessian of w . F


def hessian_matrix_part_path(out):
    return out[:-3] + ".hess.so"


def build_hessian_matrix_part(header_source, force=False):
    """``ogk_exact_hess`` / ``ogk_exact_hess_batch`` (``OGK_PART=11``) -> path of ``<module>.hess.so``.  A part of its
    own, built when an assembled Hessian is first asked for (``HipEngine.hessian_matrix``, ``BatchSweep.hessian_matrix``):
    the module and the other on-demand parts are what they were, and a user who never asks builds and loads what they
    did before.  (``hessian_part_path`` and ``.hvp.so`` stay the Hessian-vector part's.)"""
    return _build_on_demand_part(header_source, HESSIAN_MATRIX_PART, hessian_matrix_part_path, force)


PP_PART = 12                    # OGK_PART_PP, <module>.pp.so: exact second derivatives of w . F in the parameters


def pp_part_path(out):
    return out[:-3] + ".pp.so"


def build_pp_part(header_source, force=False):
    """``ogk_exact_pp`` / ``ogk_exact_pp_batch`` (``OGK_PART=12``) -> path of ``<module>.pp.so``.  A part of its own,
    built when a parameter Hessian is first asked for (``HipEngine.parameter_hessian``,
    ``BatchSweep.parameter_hessian``): the module and the other on-demand parts are what they were, and a user who never
    asks builds and loads what they did before."""
    return _build_on_demand_part(header_source, PP_PART, pp_part_path, force)


def build_module(header_source, digest=None, force=False, out_suffix="", parts=None):
    """Compile the sweep kernels against one generated header -> path of the module (its part 0; the other
    parts are built next to it, in parallel).  ``out_suffix``: write the result next to the cached module instead
    of over it (cold-start measurements: ``force=True``).  ``OG_MODULE_PARTS=1`` builds one translation unit."""
    os.makedirs(JITDIR, exist_ok=True)
    digest = module_digest(header_source)
    out = module_path(digest)
    if out_suffix:
        out = out[:-3] + out_suffix + ".so"
    kernels = os.path.join(CSRC, "ogk_kernels.hip")
    split = os.environ.get("OG_MODULE_PARTS", "") != "1" if parts is None else bool(parts)
    wanted = [part_path(out, i) for i in range(len(MODULE_PARTS))] if split else [out]
    # <module>.so is part 0 of a split build or a whole module, and only a stamp file tells which: a one-piece request
    # must not take a part 0 left by a split (or interrupted) build for the whole thing
    whole_stamp = out + ".whole"
    cached = all(os.path.exists(path) for path in wanted) and (split or os.path.exists(whole_stamp))
    if split and os.path.exists(whole_stamp) and os.path.exists(out):
        cached = True                   # a whole module serves a split request too: it holds every kernel
    if not force and cached:
        return out
    header = _write_header(header_source, digest)

    def compile_part(index):
        """-> (temporary file, target); the caller renames, in an order a concurrent reader can rely on"""
        target = wanted[index]
        tmp = target + ".tmp%d" % os.getpid()
        define = ["-DOGK_PART=%d" % MODULE_PARTS[index]] if split else []
        _run([hipcc()] + HIP_FLAGS + MODULE_FLAGS + define + ["-I" + CSRC, "-DOG_GEN_HEADER=\"%s\"" % header, kernels, "-o", tmp])
        return tmp, target

    if not split:
        for stale in (part_path(out, i) for i in range(1, len(MODULE_PARTS))):      # a one-piece module has no parts
            if os.path.exists(stale):
                os.remove(stale)
        if os.path.exists(whole_stamp):
            os.remove(whole_stamp)
        os.replace(*compile_part(0))
        with open(whole_stamp, "w") as fh:
            fh.write(digest + "\n")
        return out
    if os.path.exists(whole_stamp):
        os.remove(whole_stamp)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=len(wanted)) as pool:
        built = list(pool.map(compile_part, range(len(wanted))))
    # every part is compiled before any lands; parts 1.. first and part 0 last: a reader that finds <module>.so finds
    # its parts (the loader opens <module>.so and then looks for the parts next to it)
    for tmp, target in built[1:] + built[:1]:
        os.replace(tmp, target)
    return out
