"""Host-side ASan exercise of liblsr's C ABI (SURVEY §5 "Race detection / sanitizers").

Run with the host-ASan build (make -C langsplatv2_amd/csrc asan) and clang's ASan
runtime preloaded (tests/test_asan.py does both).  No GPU: every call below is
rejected by the host-side validation, or is pure host code (stage-name parsing,
the profiling tables, version queries), before any HIP call.  Prints "ok N" with
the number of calls made; any ASan report aborts the process."""
import ctypes
import importlib.util
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("_lsr_lib", os.path.join(HERE, "..", "langsplatv2_amd", "_lib.py"))
L = importlib.util.module_from_spec(spec)
spec.loader.exec_module(L)   # ctypes structures only; torch is never imported
lib = L.load(os.environ["LSR_LIB"])

rng = random.Random(0)
EINVAL, EUNSUP = 1, 2
calls = 0
buf = (ctypes.c_float * 64)()
P = ctypes.cast(buf, ctypes.c_void_p).value   # a valid host address used as a stand-in pointer (never dereferenced)
ALLOC = L.ALLOC_FN(lambda ctx, n, which: 0)


def settings(**kw):
    d = dict(image_height=64, image_width=64, tanfovx=0.5, tanfovy=0.5, bg=P, scale_modifier=1.0, viewmatrix=P,
             projmatrix=P, sh_degree=3, campos=P, prefiltered=0, debug=0, include_feature=0, quick_render=0,
             quick_dim=0)
    d.update(kw)
    return L.Settings(**d)


def inputs(**kw):
    d = dict(P=10, max_coeffs=16, lang_dim=0, quick_k=0, quick_index_dtype=0, means3D=P, shs=P, colors_precomp=None,
             opacities=P, scales=P, rotations=P, cov3D_precomp=None, language_feature_precomp=None,
             language_feature_weights_quick=None, language_feature_indices=None)
    d.update(kw)
    return L.Inputs(**d)


# forward: every case fails validation (expected code), so no HIP call is made
bad = [
    (dict(image_height=0), {}), (dict(image_width=-3), {}), (dict(bg=None), {}), (dict(campos=None), {}),
    ({}, dict(P=-1)), ({}, dict(means3D=None)), ({}, dict(colors_precomp=P)), ({}, dict(shs=None)),
    ({}, dict(cov3D_precomp=P)), ({}, dict(scales=None)), (dict(sh_degree=4), {}), (dict(sh_degree=-1), {}),
    ({}, dict(max_coeffs=3)), (dict(include_feature=1), dict(lang_dim=16)),
    (dict(quick_render=1), dict(quick_k=4)), (dict(quick_render=1), dict(quick_k=4, language_feature_weights_quick=P,
                                                                          language_feature_indices=P,
                                                                          quick_index_dtype=7)),
]
for skw, ikw in bad:
    out = L.FwdOut(P, P, P)
    rc = lib.lsr_forward(ctypes.byref(settings(**skw)), ctypes.byref(inputs(**ikw)), ctypes.byref(out), ALLOC, None,
                         None)
    assert rc == EINVAL, (skw, ikw, rc)
    calls += 1
# unsupported shapes
for skw, ikw in [({}, dict(max_coeffs=25, sh_degree=3)),
                 (dict(include_feature=1), dict(lang_dim=1000, language_feature_precomp=P)),
                 (dict(quick_render=1, quick_dim=100000), dict(quick_k=4, language_feature_weights_quick=P,
                                                               language_feature_indices=P))]:
    rc = lib.lsr_forward(ctypes.byref(settings(**skw)), ctypes.byref(inputs(**ikw)), ctypes.byref(L.FwdOut(P, P, P)),
                         ALLOC, None, None)
    assert rc in (EINVAL, EUNSUP), (skw, ikw, rc)
    calls += 1
# null structs / outputs
assert lib.lsr_forward(None, None, None, ALLOC, None, None) == EINVAL
assert lib.lsr_forward(ctypes.byref(settings()), ctypes.byref(inputs()), ctypes.byref(L.FwdOut(None, P, P)), ALLOC,
                       None, None) == EINVAL
calls += 2
# backward: missing workspaces / upstream gradients, quick/dense conflicts
for bkw, okw, skw in [(dict(geom=None), {}, {}), (dict(dL_dout_color=None), {}, {}), (dict(image=None), {}, {}),
                      ({}, dict(dL_dlang_weights=P), {}),
                      ({}, dict(dL_dlang=P), dict(quick_render=1))]:
    b = dict(geom=P, binning=P, image=P, num_rendered=0, radii=P, dL_dout_color=P, dL_dout_lang=None)
    b.update(bkw)
    o = L.BwdOut(**okw)
    ikw = dict(quick_k=4, language_feature_weights_quick=P, language_feature_indices=P) if skw else {}
    rc = lib.lsr_backward(ctypes.byref(settings(**skw)), ctypes.byref(inputs(**ikw)), ctypes.byref(L.BwdIn(**b)),
                          ctypes.byref(o), ALLOC, None, None)
    assert rc == EINVAL, (bkw, okw, skw, rc)
    calls += 1
# the other entry points' argument checks
assert lib.lsr_mark_visible(-1, None, None, None, None, None) == EINVAL
assert lib.lsr_quick_decode(None, None, 3, 64, 500, 4, 4, 1, 1e-10, None, ALLOC, None, None) == EINVAL
assert lib.lsr_quick_decode(None, None, 3, 32, 512, 4, 4, 1, 1e-10, None, ALLOC, None, None) == EUNSUP
assert lib.lsr_quick_decode_plan_bytes(3, 32, 512, 1) == 0 and lib.lsr_quick_decode_plan_bytes(3, 64, 512, 1) > 0
assert lib.lsr_quick_decode_prepare(None, -1, 64, 512, 1, None, None) == EINVAL
assert lib.lsr_quick_decode_run(None, 0, None, 3, 64, 17, 4, 4, 1, 1e-10, None, None) == EINVAL
assert lib.lsr_quick_decode_run(None, 2, None, 3, 64, 16, 4, 4, 1, 1e-10, None, None) == EINVAL
assert lib.lsr_knn_dist2(None, -5, None, ALLOC, None, None) == EINVAL
assert lib.lsr_adam_step(None, None, None, None, -1, 0.1, 0.9, 0.999, 1e-8, 0.0, 1, None) == EINVAL
calls += 9
# The return-code table of the single-kernel entry points: (function, arguments,
# expected code), every call rejected -- or a no-op -- before any HIP call.  The
# codes, and which of two failing checks wins ("both"), are part of the ABI's
# behaviour; tests/test_api_codes.py runs this table against the regular build.
OK, ENOMEM = 0, 4
NOALLOC = L.ALLOC_FN()   # a NULL allocator
ODD = P + 4              # a pointer that is not 16-B aligned
NAN = float("nan")
P4, I4 = ctypes.c_void_p * 4, ctypes.c_int32 * 4   # lsr_mask_segmaps' host arrays of four levels
TABLE = [
    # lsr_quick_decode(wmap, cb, L, K, Df, H, W, normalize, eps, out, alloc, ctx, stream)
    ("lsr_quick_decode", (None, None, 3, 32, 500, 4, 4, 1, 1e-10, None, ALLOC, None, None), EINVAL),   # both
    ("lsr_quick_decode", (None, None, 3, 64, 0, 4, 4, 1, 1e-10, None, ALLOC, None, None), EINVAL),
    ("lsr_quick_decode", (None, None, 0, 64, 512, 4, 4, 1, 1e-10, None, ALLOC, None, None), OK),
    ("lsr_quick_decode", (None, None, 3, 64, 512, 4, 4, 1, 1e-10, None, ALLOC, None, None), EINVAL),
    ("lsr_quick_decode", (P, P, 3, 64, 512, 4, 4, 1, 1e-10, P, NOALLOC, None, None), EINVAL),
    ("lsr_quick_decode", (P, P, 3, 64, 512, 4, 4, 1, 1e-10, P, ALLOC, None, None), ENOMEM),
    # lsr_quick_decode_prepare(cb, L, K, Df, normalize, plan, stream)
    ("lsr_quick_decode_prepare", (None, 3, 32, 512, 1, None, None), EUNSUP),
    ("lsr_quick_decode_prepare", (None, 3, 32, 8, 1, None, None), EINVAL),   # both
    ("lsr_quick_decode_prepare", (None, 0, 64, 512, 1, None, None), OK),
    ("lsr_quick_decode_prepare", (P, 3, 64, 512, 1, None, None), EINVAL),
    # lsr_quick_decode_run(wmap, layout, plan, L, K, Df, H, W, normalize, eps, out, stream)
    ("lsr_quick_decode_run", (None, 0, None, 3, 32, 512, 4, 4, 1, 1e-10, None, None), EUNSUP),
    ("lsr_quick_decode_run", (None, 2, None, 3, 32, 512, 4, 4, 1, 1e-10, None, None), EINVAL),   # both
    ("lsr_quick_decode_run", (None, 0, None, 3, 32, 17, 4, 4, 1, 1e-10, None, None), EINVAL),    # both
    ("lsr_quick_decode_run", (None, 1, None, 0, 64, 512, 4, 4, 1, 1e-10, None, None), OK),
    ("lsr_quick_decode_run", (None, 0, None, 3, 64, 512, 0, 4, 1, 1e-10, None, None), OK),
    ("lsr_quick_decode_run", (None, 0, None, 3, 64, 512, 4, 4, 1, 1e-10, None, None), EINVAL),
    ("lsr_quick_decode_run", (P, 1, P, 3, 64, 1024, 4, 4, 1, 1e-10, P, None), EUNSUP),
    ("lsr_quick_decode_run", (ODD, 1, P, 3, 64, 512, 4, 4, 1, 1e-10, P, None), EUNSUP),
    ("lsr_quick_decode_run", (ODD, 1, P, 3, 64, 512, 4, -1, 1, 1e-10, P, None), EINVAL),
    # lsr_quick_pack_codes(indices, dtype, N, K, quick_dim, packed, stream)
    ("lsr_quick_pack_codes", (None, 0, -1, 12, 192, None, None), EINVAL),
    ("lsr_quick_pack_codes", (None, 3, 10, 12, 192, None, None), EINVAL),
    ("lsr_quick_pack_codes", (None, 3, 10, 8, 192, None, None), EINVAL),    # both
    ("lsr_quick_pack_codes", (None, 0, 10, 12, -1, None, None), EINVAL),
    ("lsr_quick_pack_codes", (None, 0, 10, 8, 192, None, None), EUNSUP),
    ("lsr_quick_pack_codes", (None, 1, 10, 12, 256, None, None), EUNSUP),
    ("lsr_quick_pack_codes", (None, 2, 0, 12, 0, None, None), OK),
    ("lsr_quick_pack_codes", (None, 2, 0, 13, 0, None, None), EUNSUP),      # K before the no-op
    ("lsr_quick_pack_codes", (None, 0, 10, 12, 192, P, None), EINVAL),
    ("lsr_quick_pack_codes", (P, 0, 10, 12, 192, ODD, None), EINVAL),
    # lsr_quick_query_prepare(cb, pos, neg, L, K, Df, n_pos, n_neg, plan, stream)
    ("lsr_quick_query_prepare", (None, None, None, 3, 64, 17, 1, 1, None, None), EINVAL),
    ("lsr_quick_query_prepare", (None, None, None, 3, 64, 512, 0, 1, None, None), EINVAL),
    ("lsr_quick_query_prepare", (None, None, None, -1, 64, 512, 1, 1, None, None), EINVAL),
    ("lsr_quick_query_prepare", (None, None, None, 3, 32, 512, 1, 1, None, None), EUNSUP),
    ("lsr_quick_query_prepare", (None, None, None, 3, 64, 512, 33, 32, None, None), EUNSUP),
    ("lsr_quick_query_prepare", (None, None, None, 3, 32, 17, 1, 1, None, None), EINVAL),   # both
    ("lsr_quick_query_prepare", (None, None, None, 0, 64, 512, 1, 1, None, None), OK),
    ("lsr_quick_query_prepare", (None, None, None, 3, 64, 512, 1, 1, None, None), EINVAL),
    ("lsr_quick_query_prepare", (P, P, None, 3, 64, 512, 1, 1, P, None), EINVAL),
    # lsr_quick_query_run(wmap, layout, plan, L, K, n_pos, n_neg, H, W, mode, scale, eps, out, stream)
    ("lsr_quick_query_run", (None, 2, None, 3, 64, 1, 1, 4, 4, 0, 10.0, 1e-10, None, None), EINVAL),
    ("lsr_quick_query_run", (None, 0, None, 3, 64, 1, 1, 4, 4, 2, 10.0, 1e-10, None, None), EINVAL),
    ("lsr_quick_query_run", (None, 0, None, 3, 64, 1, 1, 4, 4, 0, -1.0, 1e-10, None, None), EINVAL),
    ("lsr_quick_query_run", (None, 0, None, 3, 64, 1, 1, 4, 4, 0, NAN, 1e-10, None, None), EINVAL),
    ("lsr_quick_query_run", (None, 0, None, 3, 64, 0, 1, 4, 4, 0, 10.0, 1e-10, None, None), EINVAL),
    ("lsr_quick_query_run", (None, 0, None, 3, 32, 1, 1, 4, 4, 0, 10.0, 1e-10, None, None), EUNSUP),
    ("lsr_quick_query_run", (None, 0, None, 3, 64, 1, 0, 4, 4, 0, 10.0, 1e-10, None, None), EUNSUP),
    ("lsr_quick_query_run", (None, 0, None, 3, 64, 40, 30, 4, 4, 1, 10.0, 1e-10, None, None), EUNSUP),
    ("lsr_quick_query_run", (None, 5, None, 3, 32, 1, 1, 4, 4, 0, 10.0, 1e-10, None, None), EINVAL),   # both
    ("lsr_quick_query_run", (None, 0, None, 3, 32, 1, 0, 4, 4, 0, -1.0, 1e-10, None, None), EINVAL),   # both
    ("lsr_quick_query_run", (None, 0, None, 3, 64, 1, 0, 0, 4, 0, 10.0, 1e-10, None, None), EUNSUP),   # before the no-op
    ("lsr_quick_query_run", (None, 0, None, 3, 64, 1, 1, 0, 4, 0, 10.0, 1e-10, None, None), OK),
    ("lsr_quick_query_run", (None, 1, None, 0, 64, 1, 0, 4, 4, 1, -1.0, 1e-10, None, None), OK),
    ("lsr_quick_query_run", (None, 0, None, 3, 64, 1, 1, 4, 4, 0, 10.0, 1e-10, None, None), EINVAL),
    ("lsr_quick_query_run", (ODD, 1, P, 3, 64, 1, 1, 4, 4, 0, 10.0, 1e-10, P, None), EUNSUP),
    # lsr_quick_heat_prepare(cb, pos, neg, L, K, Df, n_pos, n_neg, plan, stream)
    ("lsr_quick_heat_prepare", (None, None, None, 3, 64, 17, 1, 1, None, None), EINVAL),
    ("lsr_quick_heat_prepare", (None, None, None, 3, 64, 512, 0, 1, None, None), EINVAL),
    ("lsr_quick_heat_prepare", (None, None, None, 3, 32, 512, 1, 1, None, None), EUNSUP),
    ("lsr_quick_heat_prepare", (None, None, None, 4, 64, 512, 1, 1, None, None), EUNSUP),
    ("lsr_quick_heat_prepare", (None, None, None, 3, 64, 512, 33, 32, None, None), EUNSUP),
    ("lsr_quick_heat_prepare", (None, None, None, 4, 64, 17, 1, 1, None, None), EINVAL),   # both
    ("lsr_quick_heat_prepare", (None, None, None, 0, 64, 512, 1, 1, None, None), OK),
    ("lsr_quick_heat_prepare", (None, None, None, 3, 64, 512, 1, 1, None, None), EINVAL),
    ("lsr_quick_heat_prepare", (P, P, None, 3, 64, 512, 1, 1, P, None), EINVAL),
    # lsr_quick_heat_run(wmap, layout, plan, L, K, n_pos, n_neg, H, W, mode, scale, eps, out, stream)
    ("lsr_quick_heat_run", (None, 2, None, 3, 64, 1, 1, 4, 4, 0, 10.0, 1e-10, None, None), EINVAL),
    ("lsr_quick_heat_run", (None, 0, None, 3, 64, 1, 1, 4, 4, 2, 10.0, 1e-10, None, None), EINVAL),
    ("lsr_quick_heat_run", (None, 0, None, 3, 64, 1, 1, 4, 4, 1, -1.0, 1e-10, None, None), EINVAL),
    ("lsr_quick_heat_run", (None, 0, None, 3, 64, 1, 0, 4, 4, 0, NAN, 1e-10, None, None), EINVAL),
    ("lsr_quick_heat_run", (None, 0, None, 3, 64, 0, 1, 4, 4, 0, 10.0, 1e-10, None, None), EINVAL),
    ("lsr_quick_heat_run", (None, 0, None, 3, 32, 1, 1, 4, 4, 0, 10.0, 1e-10, None, None), EUNSUP),
    ("lsr_quick_heat_run", (None, 0, None, 4, 64, 1, 1, 4, 4, 0, 10.0, 1e-10, None, None), EUNSUP),
    ("lsr_quick_heat_run", (None, 0, None, 3, 64, 1, 0, 4, 4, 1, 10.0, 1e-10, None, None), EUNSUP),
    ("lsr_quick_heat_run", (None, 0, None, 3, 64, 40, 30, 4, 4, 0, 10.0, 1e-10, None, None), EUNSUP),
    ("lsr_quick_heat_run", (None, 5, None, 4, 64, 1, 1, 4, 4, 0, 10.0, 1e-10, None, None), EINVAL),   # both
    ("lsr_quick_heat_run", (None, 0, None, 4, 64, 1, 1, 0, 4, 0, 10.0, 1e-10, None, None), EUNSUP),   # before the no-op
    ("lsr_quick_heat_run", (None, 0, None, 3, 64, 1, 0, 0, 4, 0, 0.0, 1e-10, None, None), OK),
    ("lsr_quick_heat_run", (None, 1, None, 0, 64, 1, 1, 4, 4, 1, 10.0, 1e-10, None, None), OK),
    ("lsr_quick_heat_run", (None, 0, None, 3, 64, 1, 0, 4, 4, 0, 0.0, 1e-10, None, None), EINVAL),
    ("lsr_quick_heat_run", (ODD, 1, P, 3, 64, 1, 0, 4, 4, 0, 0.0, 1e-10, P, None), EUNSUP),
    # lsr_heat_frame(maps, stats, rgb, lut, planes, H, W, curve, threshold, min_range, alpha, out, stream)
    ("lsr_heat_frame", (None, None, None, None, -1, 4, 4, 0, 0.22, 0.02, 0.5, None, None), EINVAL),
    ("lsr_heat_frame", (None, None, None, None, 1, 4, 4, 2, 0.22, 0.02, 0.5, None, None), EINVAL),
    ("lsr_heat_frame", (None, None, None, None, 1, 4, 4, 0, 0.22, 0.02, -0.1, None, None), EINVAL),
    ("lsr_heat_frame", (None, None, None, None, 1, 4, 4, 1, 0.22, 0.02, 1.5, None, None), EINVAL),
    ("lsr_heat_frame", (None, None, None, None, 1, 4, 4, 0, 0.22, 0.02, NAN, None, None), EINVAL),
    ("lsr_heat_frame", (None, None, None, None, 70000, 4, 4, 0, 0.22, 0.02, 0.5, None, None), EUNSUP),
    ("lsr_heat_frame", (None, None, None, None, 1, 65536, 65536, 0, 0.22, 0.02, 0.5, None, None), EUNSUP),
    ("lsr_heat_frame", (None, None, None, None, 70000, 4, 4, 0, 0.22, 0.02, 2.0, None, None), EINVAL),   # both
    ("lsr_heat_frame", (None, None, None, None, 0, 4, 4, 1, 0.22, 0.0, 1.0, None, None), OK),
    ("lsr_heat_frame", (None, None, None, None, 2, 4, 0, 0, 0.22, 0.02, 0.0, None, None), OK),
    ("lsr_heat_frame", (None, None, None, None, 1, 4, 4, 0, 0.22, 0.02, 0.5, None, None), EINVAL),
    ("lsr_heat_frame", (P, P, None, P, 1, 4, 4, 0, 0.22, 0.02, 0.5, None, None), EINVAL),
    # lsr_quick_semantic_prepare(cb, labels, neg, L, K, Df, n_labels, n_neg, plan, stream)
    ("lsr_quick_semantic_prepare", (None, None, None, 3, 64, 512, 0, 4, None, None), EINVAL),
    ("lsr_quick_semantic_prepare", (None, None, None, 3, 64, 512, 5, -1, None, None), EINVAL),
    ("lsr_quick_semantic_prepare", (None, None, None, -1, 64, 512, 5, 4, None, None), EINVAL),
    ("lsr_quick_semantic_prepare", (None, None, None, 3, 64, 0, 5, 4, None, None), EINVAL),
    ("lsr_quick_semantic_prepare", (None, None, None, 3, 32, 512, 5, 4, None, None), EUNSUP),
    ("lsr_quick_semantic_prepare", (None, None, None, 3, 64, 17, 5, 4, None, None), EUNSUP),
    ("lsr_quick_semantic_prepare", (None, None, None, 3, 64, 512, 253, 4, None, None), EUNSUP),
    ("lsr_quick_semantic_prepare", (None, None, None, 3, 32, 512, 0, 4, None, None), EINVAL),   # both
    ("lsr_quick_semantic_prepare", (None, None, None, 0, 64, 512, 5, 4, None, None), OK),
    ("lsr_quick_semantic_prepare", (None, None, None, 3, 64, 512, 5, 4, None, None), EINVAL),
    ("lsr_quick_semantic_prepare", (P, P, None, 3, 64, 512, 5, 4, P, None), EINVAL),    # negatives without their rows
    # lsr_quick_semantic_run(wmap, layout, plan, L, K, n_labels, n_neg, H, W, scale, eps, labels, scores, stream)
    ("lsr_quick_semantic_run", (None, 2, None, 3, 64, 5, 4, 4, 4, 10.0, 1e-10, None, None, None), EINVAL),
    ("lsr_quick_semantic_run", (None, 0, None, 3, 64, 5, 4, 4, 4, -1.0, 1e-10, None, None, None), EINVAL),
    ("lsr_quick_semantic_run", (None, 0, None, 3, 64, 5, 4, 4, 4, NAN, 1e-10, None, None, None), EINVAL),
    ("lsr_quick_semantic_run", (None, 0, None, 3, 64, 0, 4, 4, 4, 10.0, 1e-10, None, None, None), EINVAL),
    ("lsr_quick_semantic_run", (None, 0, None, 3, 64, 5, 4, -1, 4, 10.0, 1e-10, None, None, None), EINVAL),
    ("lsr_quick_semantic_run", (None, 0, None, 3, 32, 5, 4, 4, 4, 10.0, 1e-10, None, None, None), EUNSUP),
    ("lsr_quick_semantic_run", (None, 0, None, 3, 64, 253, 4, 4, 4, 10.0, 1e-10, None, None, None), EUNSUP),
    ("lsr_quick_semantic_run", (None, 0, None, 3, 32, 5, 4, 4, 4, -1.0, 1e-10, None, None, None), EINVAL),   # both
    ("lsr_quick_semantic_run", (None, 0, None, 3, 64, 253, 4, 0, 4, 10.0, 1e-10, None, None, None), EUNSUP),   # before the no-op
    ("lsr_quick_semantic_run", (None, 0, None, 3, 64, 5, 4, 0, 4, 10.0, 1e-10, None, None, None), OK),
    ("lsr_quick_semantic_run", (None, 1, None, 0, 64, 5, 0, 4, 4, 0.0, 1e-10, None, None, None), OK),
    ("lsr_quick_semantic_run", (None, 0, None, 3, 64, 5, 4, 4, 4, 10.0, 1e-10, None, None, None), EINVAL),
    ("lsr_quick_semantic_run", (P, 0, P, 3, 64, 5, 4, 4, 4, 10.0, 1e-10, None, P, None), EINVAL),      # scores without labels
    ("lsr_quick_semantic_run", (ODD, 1, P, 3, 64, 5, 4, 4, 4, 10.0, 1e-10, P, None, None), EUNSUP),
    # lsr_semantic_merge(labels, scores, L, H, W, out, level, stream)
    ("lsr_semantic_merge", (None, None, -1, 4, 4, None, None, None), EINVAL),
    ("lsr_semantic_merge", (None, None, 256, 4, 4, None, None, None), EUNSUP),
    ("lsr_semantic_merge", (None, None, 3, 65536, 65536, None, None, None), EUNSUP),
    ("lsr_semantic_merge", (None, None, 256, 4, -1, None, None, None), EINVAL),   # both
    ("lsr_semantic_merge", (None, None, 0, 4, 4, None, None, None), OK),
    ("lsr_semantic_merge", (None, None, 3, 4, 0, None, None, None), OK),
    ("lsr_semantic_merge", (None, None, 3, 4, 4, None, None, None), EINVAL),
    ("lsr_semantic_merge", (P, P, 3, 4, 4, None, P, None), EINVAL),
    # lsr_semantic_confusion(pred, gt, P, H, W, n_classes, counts, stream)
    ("lsr_semantic_confusion", (None, None, 3, 4, 4, 0, None, None), EINVAL),
    ("lsr_semantic_confusion", (None, None, -1, 4, 4, 21, None, None), EINVAL),
    ("lsr_semantic_confusion", (None, None, 3, 4, 4, 257, None, None), EUNSUP),
    ("lsr_semantic_confusion", (None, None, 65536, 4, 4, 21, None, None), EUNSUP),
    ("lsr_semantic_confusion", (None, None, 3, 65536, 65536, 21, None, None), EUNSUP),
    ("lsr_semantic_confusion", (None, None, 0, 4, 4, 257, None, None), EUNSUP),   # before the no-op
    ("lsr_semantic_confusion", (None, None, 0, 4, 4, 21, None, None), OK),
    ("lsr_semantic_confusion", (None, None, 3, 0, 4, 256, None, None), OK),
    ("lsr_semantic_confusion", (None, None, 3, 4, 4, 21, None, None), EINVAL),
    ("lsr_semantic_confusion", (P, P, 3, 4, 4, 21, None, None), EINVAL),
    # lsr_query_smooth(rel, planes, H, W, kernel, avg, blend, stats, loc, workspace, stream)
    ("lsr_query_smooth", (None, 2, 4, 4, 4, None, None, None, None, None, None), EINVAL),
    ("lsr_query_smooth", (None, 2, 4, 4, 0, None, None, None, None, None, None), EINVAL),
    ("lsr_query_smooth", (None, -1, 4, 4, 3, None, None, None, None, None, None), EINVAL),
    ("lsr_query_smooth", (None, 2, 4, 4, 65, None, None, None, None, None, None), EUNSUP),
    ("lsr_query_smooth", (None, 65536, 4, 4, 3, None, None, None, None, None, None), EUNSUP),
    ("lsr_query_smooth", (None, 2, 65536, 65536, 3, None, None, None, None, None, None), EUNSUP),
    ("lsr_query_smooth", (None, 2, 4, 4, 66, None, None, None, None, None, None), EINVAL),   # both
    ("lsr_query_smooth", (None, 0, 4, 4, 65, None, None, None, None, None, None), EUNSUP),   # before the no-op
    ("lsr_query_smooth", (None, 0, 4, 4, 3, None, None, None, None, None, None), OK),
    ("lsr_query_smooth", (None, 2, 4, 0, 63, None, None, None, None, None, None), OK),
    ("lsr_query_smooth", (None, 2, 4, 4, 3, None, None, None, None, None, None), EINVAL),
    ("lsr_query_smooth", (P, 2, 4, 4, 3, None, None, P, P, None, None), EINVAL),
    # lsr_query_mask(blend, stats, gt, planes, n_prompt, H, W, thresh, smooth_kernel, mask, counts, masked_sum,
    #                workspace, stream)
    ("lsr_query_mask", (None, None, None, 2, 1, 4, 4, 0.5, 2, None, None, None, None, None), EINVAL),
    ("lsr_query_mask", (None, None, P, 2, 0, 4, 4, 0.5, 3, None, None, None, None, None), EINVAL),
    ("lsr_query_mask", (None, None, P, 3, 2, 4, 4, 0.5, 3, None, None, None, None, None), EINVAL),
    ("lsr_query_mask", (None, None, None, 2, 1, 4, 4, 0.5, 17, None, None, None, None, None), EUNSUP),
    ("lsr_query_mask", (None, None, None, 70000, 1, 4, 4, 0.5, 3, None, None, None, None, None), EUNSUP),
    ("lsr_query_mask", (None, None, P, 2, 0, 4, 4, 0.5, 17, None, None, None, None, None), EINVAL),   # both
    ("lsr_query_mask", (None, None, None, 2, 1, 4, 4, 0.5, 18, None, None, None, None, None), EINVAL),   # both
    ("lsr_query_mask", (None, None, None, 2, 0, 4, 0, 0.5, 3, None, None, None, None, None), OK),
    ("lsr_query_mask", (None, None, None, 0, 1, 4, 4, 0.5, 15, None, None, None, None, None), OK),
    ("lsr_query_mask", (None, None, None, 2, 1, 4, 4, 0.5, 3, None, None, None, None, None), EINVAL),
    ("lsr_query_mask", (P, P, None, 2, 1, 4, 4, 0.5, 3, P, P, P, None, None), EINVAL),
    # lsr_lang_loss_forward(wmap, cb, K, Df, H, W, seg, feat, S, loss, pixel_stats, alloc, ctx, stream):
    # an empty image is an error here, not a no-op
    ("lsr_lang_loss_forward", (P, P, 0, 512, 4, 4, P, P, 2, P, None, ALLOC, None, None), EINVAL),
    ("lsr_lang_loss_forward", (P, P, 64, 512, 0, 4, P, P, 2, P, None, ALLOC, None, None), EINVAL),
    ("lsr_lang_loss_forward", (P, P, 32, 512, 4, 4, P, P, 2, P, None, ALLOC, None, None), EUNSUP),
    ("lsr_lang_loss_forward", (P, P, 64, 24, 4, 4, P, P, 2, P, None, ALLOC, None, None), EUNSUP),
    ("lsr_lang_loss_forward", (P, P, 32, 512, 4, 4, P, P, -1, P, None, ALLOC, None, None), EINVAL),   # both
    ("lsr_lang_loss_forward", (None, P, 32, 512, 4, 4, P, P, 2, P, None, ALLOC, None, None), EUNSUP),  # both
    ("lsr_lang_loss_forward", (None, P, 64, 512, 4, 4, P, P, 2, P, None, ALLOC, None, None), EINVAL),
    ("lsr_lang_loss_forward", (P, P, 64, 512, 4, 4, P, None, 2, P, None, ALLOC, None, None), EINVAL),
    ("lsr_lang_loss_forward", (P, P, 64, 512, 4, 4, P, None, 0, None, None, ALLOC, None, None), EINVAL),
    ("lsr_lang_loss_forward", (P, P, 64, 512, 4, 4, P, P, 2, P, None, NOALLOC, None, None), EINVAL),
    ("lsr_lang_loss_forward", (P, P, 64, 512, 4, 4, P, None, 0, None, P, ALLOC, None, None), ENOMEM),
    # lsr_lang_loss_backward(wmap, cb, K, Df, H, W, seg, feat, S, pixel_stats, grad_loss, grad_wmap, grad_cb,
    #                        alloc, ctx, stream)
    ("lsr_lang_loss_backward", (P, P, 64, 0, 4, 4, P, P, 2, None, P, P, P, ALLOC, None, None), EINVAL),
    ("lsr_lang_loss_backward", (P, P, 64, 512, 4, -4, P, P, 2, None, P, P, P, ALLOC, None, None), EINVAL),
    ("lsr_lang_loss_backward", (P, P, 128, 512, 4, 4, P, P, 2, None, P, P, P, ALLOC, None, None), EUNSUP),
    ("lsr_lang_loss_backward", (P, P, 128, 520, 0, 4, P, P, 2, None, P, P, P, ALLOC, None, None), EINVAL),   # both
    ("lsr_lang_loss_backward", (P, P, 64, 520, 4, 4, P, P, 2, None, None, P, P, ALLOC, None, None), EUNSUP),  # both
    ("lsr_lang_loss_backward", (P, P, 64, 512, 4, 4, None, P, 2, None, P, P, P, ALLOC, None, None), EINVAL),
    ("lsr_lang_loss_backward", (P, P, 64, 512, 4, 4, P, P, 2, None, None, P, P, ALLOC, None, None), EINVAL),
    ("lsr_lang_loss_backward", (P, P, 64, 512, 4, 4, P, P, 2, None, P, P, None, ALLOC, None, None), EINVAL),
    ("lsr_lang_loss_backward", (P, P, 64, 512, 4, 4, P, P, 2, None, P, P, P, NOALLOC, None, None), EINVAL),
    ("lsr_lang_loss_backward", (P, P, 64, 512, 4, 4, P, P, 2, P, P, P, P, ALLOC, None, None), ENOMEM),
    # lsr_topk_code_forward(logits, N, L, K, k, dense, sparse_w, sparse_idx, idx_dtype, level_offset, stream)
    ("lsr_topk_code_forward", (None, 10, 1, 320, 4, None, None, None, 0, 0, None), EUNSUP),
    ("lsr_topk_code_forward", (None, 10, 1, 48, 0, None, None, None, 7, 0, None), EUNSUP),   # both
    ("lsr_topk_code_forward", (None, 10, 1, 0, 4, None, None, None, 0, 0, None), EINVAL),
    ("lsr_topk_code_forward", (None, 10, 1, -64, 4, None, None, None, 0, 0, None), EINVAL),
    ("lsr_topk_code_forward", (None, 10, 1, 64, 4, None, None, None, 3, 0, None), EINVAL),
    ("lsr_topk_code_forward", (None, 0, 1, 64, 4, None, None, None, -1, 0, None), EINVAL),   # dtype before the no-op
    # lsr_topk_code_backward(logits, grad_dense, N, L, K, k, grad_logits, stream)
    ("lsr_topk_code_backward", (None, None, 10, 1, 100, 4, None, None), EUNSUP),
    ("lsr_topk_code_backward", (None, None, 10, 0, 64, 4, None, None), EINVAL),
    ("lsr_topk_code_backward", (None, None, 0, 3, 128, 4, None, None), OK),
    ("lsr_topk_code_backward", (P, P, 10, 3, 128, 4, None, None), EINVAL),
    # lsr_topk_code_backward_sparse(logits, grad_weights, N, L, K, k, grad_logits, stream)
    ("lsr_topk_code_backward_sparse", (None, None, 10, 1, 48, 4, None, None), EUNSUP),
    ("lsr_topk_code_backward_sparse", (None, None, 10, 1, 320, 4, None, None), EUNSUP),
    ("lsr_topk_code_backward_sparse", (None, None, 10, 1, 64, 0, None, None), EINVAL),
    ("lsr_topk_code_backward_sparse", (None, None, 10, 1, 64, 65, None, None), EINVAL),
    ("lsr_topk_code_backward_sparse", (None, None, -1, 1, 64, 4, None, None), EINVAL),
    ("lsr_topk_code_backward_sparse", (None, None, 10, 0, 64, 4, None, None), EINVAL),
    ("lsr_topk_code_backward_sparse", (None, None, 10, 1, 0, 4, None, None), EINVAL),
    ("lsr_topk_code_backward_sparse", (None, None, 1 << 30, 1, 64, 4, None, None), EINVAL),   # N L K past 2^31
    ("lsr_topk_code_backward_sparse", (None, None, 10, 1, 48, 0, None, None), EUNSUP),        # both
    ("lsr_topk_code_backward_sparse", (None, None, -1, 0, 320, 4, None, None), EUNSUP),       # both
    ("lsr_topk_code_backward_sparse", (None, None, 0, 1, 48, 4, None, None), EUNSUP),         # before the no-op
    ("lsr_topk_code_backward_sparse", (None, None, 0, 2, 256, 256, None, None), OK),
    ("lsr_topk_code_backward_sparse", (None, None, 10, 1, 64, 4, None, None), EINVAL),
    ("lsr_topk_code_backward_sparse", (P, P, 10, 1, 64, 4, None, None), EINVAL),
    # lsr_sh_grad_from_views(N, M, sh_degree, means3D, R, campos, drgb, dL_dsh, stream): no shape is
    # "unsupported" here, more than 16 coefficients are an invalid argument
    ("lsr_sh_grad_from_views", (-1, 16, 3, None, 1, None, None, None, None), EINVAL),
    ("lsr_sh_grad_from_views", (10, 0, 0, None, 1, None, None, None, None), EINVAL),
    ("lsr_sh_grad_from_views", (10, 17, 3, None, 1, None, None, None, None), EINVAL),
    ("lsr_sh_grad_from_views", (10, 25, 4, None, 1, None, None, None, None), EINVAL),
    ("lsr_sh_grad_from_views", (10, 16, 4, None, 1, None, None, None, None), EINVAL),
    ("lsr_sh_grad_from_views", (10, 9, 3, None, 1, None, None, None, None), EINVAL),
    ("lsr_sh_grad_from_views", (10, 16, 3, None, -1, None, None, None, None), EINVAL),
    ("lsr_sh_grad_from_views", (0, 17, 3, None, 1, None, None, None, None), EINVAL),   # before the no-op
    ("lsr_sh_grad_from_views", (0, 16, 3, None, 1, None, None, None, None), OK),
    ("lsr_sh_grad_from_views", (10, 16, 3, None, 0, None, None, P, None), EINVAL),
    ("lsr_sh_grad_from_views", (10, 16, 3, P, 2, None, P, P, None), EINVAL),
    ("lsr_sh_grad_from_views", (10, 16, 3, P, 2, P, None, P, None), EINVAL),
    # lsr_knn_dist2(points, N, out, alloc, ctx, stream); lsr_adam_step(p, g, m, v, n, lr, b1, b2, eps, wd, step, stream)
    ("lsr_knn_dist2", (None, 1 << 31, None, ALLOC, None, None), EINVAL),
    ("lsr_knn_dist2", (None, 0, None, ALLOC, None, None), OK),
    ("lsr_knn_dist2", (P, 10, P, NOALLOC, None, None), EINVAL),
    ("lsr_adam_step", (None, None, None, None, 10, 0.1, 0.9, 0.999, 1e-8, 0.0, 0, None), EINVAL),
    ("lsr_adam_step", (None, None, None, None, 10, 0.1, 1.0, 0.999, 1e-8, 0.0, 1, None), EINVAL),
    ("lsr_adam_step", (None, None, None, None, 10, 0.1, 0.9, NAN, 1e-8, 0.0, 1, None), EINVAL),
    ("lsr_adam_step", (None, None, None, None, 0, 0.1, 0.9, 0.999, 1e-8, 0.0, 1, None), OK),
    ("lsr_adam_step", (P, P, P, None, 10, 0.1, 0.9, 0.999, 1e-8, 0.0, 1, None), EINVAL),
    ("lsr_mark_visible", (10, None, P, P, P, None), EINVAL),
    # lsr_kmeans_prepare(centers, K, D, workspace, stream): every shape not taken is an invalid argument
    ("lsr_kmeans_prepare", (None, 64, 512, P, None), EINVAL),
    ("lsr_kmeans_prepare", (P, 64, 512, None, None), EINVAL),
    ("lsr_kmeans_prepare", (P, 0, 512, P, None), EINVAL),
    ("lsr_kmeans_prepare", (P, 257, 512, P, None), EINVAL),
    ("lsr_kmeans_prepare", (P, 64, 6, P, None), EINVAL),
    ("lsr_kmeans_prepare", (P, 64, 1028, P, None), EINVAL),
    # lsr_kmeans_assign(x, M, D, K, workspace, assign, dist, residual_out, stream)
    ("lsr_kmeans_assign", (None, 10, 512, 64, P, P, P, None, None), EINVAL),
    ("lsr_kmeans_assign", (P, 10, 512, 64, None, P, P, None, None), EINVAL),
    ("lsr_kmeans_assign", (P, 10, 512, 64, P, None, P, None, None), EINVAL),
    ("lsr_kmeans_assign", (P, 10, 512, 64, P, P, None, None, None), EINVAL),
    ("lsr_kmeans_assign", (P, 10, 512, 64, P, P, P, P, None), EINVAL),     # the residual may not alias x
    ("lsr_kmeans_assign", (P, 10, 512, 0, P, P, P, None, None), EINVAL),
    ("lsr_kmeans_assign", (P, 10, 512, 257, P, P, P, None, None), EINVAL),
    ("lsr_kmeans_assign", (P, 10, 6, 64, P, P, P, None, None), EINVAL),
    ("lsr_kmeans_assign", (P, 10, 1028, 64, P, P, P, None, None), EINVAL),
    ("lsr_kmeans_assign", (P, -1, 512, 64, P, P, P, None, None), EINVAL),
    ("lsr_kmeans_assign", (P, 1 << 31, 512, 64, P, P, P, None, None), EINVAL),
    ("lsr_kmeans_assign", (None, 0, 512, 257, None, None, None, None, None), EINVAL),   # the shape before the no-op
    ("lsr_kmeans_assign", (None, 0, 512, 64, None, None, None, None, None), OK),
    # lsr_kmeans_update(x, assign, M, D, K, workspace, centers_out, counts_out, stream)
    ("lsr_kmeans_update", (None, P, 10, 512, 64, P, P, P, None), EINVAL),
    ("lsr_kmeans_update", (P, None, 10, 512, 64, P, P, P, None), EINVAL),
    ("lsr_kmeans_update", (P, P, 10, 512, 64, None, P, P, None), EINVAL),
    ("lsr_kmeans_update", (P, P, 10, 512, 64, P, None, P, None), EINVAL),
    ("lsr_kmeans_update", (P, P, 10, 512, 64, P, P, None, None), EINVAL),
    ("lsr_kmeans_update", (P, P, 10, 512, 0, P, P, P, None), EINVAL),
    ("lsr_kmeans_update", (P, P, 10, 512, 257, P, P, P, None), EINVAL),
    ("lsr_kmeans_update", (P, P, 10, 6, 64, P, P, P, None), EINVAL),
    ("lsr_kmeans_update", (P, P, 10, 1028, 64, P, P, P, None), EINVAL),
    ("lsr_kmeans_update", (P, P, -1, 512, 64, P, P, P, None), EINVAL),
    ("lsr_kmeans_update", (None, None, 0, 6, 64, None, None, None, None), EINVAL),      # the shape before the no-op
    ("lsr_kmeans_update", (None, None, 0, 512, 64, None, None, None, None), OK),
    # lsr_mask_pack(masks, N, H, W, words, area, stream): beyond 4096 masks or 2^24 pixels is unsupported
    ("lsr_mask_pack", (None, 5, 3, 5, P, P, None), EINVAL),
    ("lsr_mask_pack", (P, 5, 3, 5, None, P, None), EINVAL),
    ("lsr_mask_pack", (P, 5, 3, 5, P, None, None), EINVAL),
    ("lsr_mask_pack", (P, 5, 3, 5, ODD, P, None), EINVAL),
    ("lsr_mask_pack", (P, -1, 3, 5, P, P, None), EINVAL),
    ("lsr_mask_pack", (P, 5, 0, 5, P, P, None), EINVAL),
    ("lsr_mask_pack", (P, 4097, 3, 5, P, P, None), EUNSUP),
    ("lsr_mask_pack", (P, 5, 4096, 4097, P, P, None), EUNSUP),
    ("lsr_mask_pack", (None, 4097, 0, 5, None, None, None), EINVAL),   # both
    ("lsr_mask_pack", (None, 0, 0, 5, None, None, None), EINVAL),      # the shape before the no-op
    ("lsr_mask_pack", (None, 0, 3, 5, None, None, None), OK),
    # lsr_mask_pair_counts(words, N, H, W, order, inter, stream)
    ("lsr_mask_pair_counts", (None, 5, 3, 5, None, P, None), EINVAL),
    ("lsr_mask_pair_counts", (P, 5, 3, 5, None, None, None), EINVAL),
    ("lsr_mask_pair_counts", (ODD, 5, 3, 5, None, P, None), EINVAL),
    ("lsr_mask_pair_counts", (P, 4097, 3, 5, None, P, None), EUNSUP),
    ("lsr_mask_pair_counts", (P, 5, 4096, 4097, None, P, None), EUNSUP),
    ("lsr_mask_pair_counts", (None, 0, 3, 5, None, None, None), OK),
    # lsr_mask_nms_select(words, area, N, H, W, order, conf, iou_thr, inner_thr, workspace, keep, criteria,
    #                     selected, count, stream)
    ("lsr_mask_nms_select", (None, P, 5, 3, 5, P, P, 0.8, 0.5, P, P, None, P, P, None), EINVAL),
    ("lsr_mask_nms_select", (P, None, 5, 3, 5, P, P, 0.8, 0.5, P, P, None, P, P, None), EINVAL),
    ("lsr_mask_nms_select", (P, P, 5, 3, 5, None, P, 0.8, 0.5, P, P, None, P, P, None), EINVAL),
    ("lsr_mask_nms_select", (P, P, 5, 3, 5, P, None, 0.8, 0.5, P, P, None, P, P, None), EINVAL),
    ("lsr_mask_nms_select", (P, P, 5, 3, 5, P, P, 0.8, 0.5, None, P, None, P, P, None), EINVAL),
    ("lsr_mask_nms_select", (P, P, 5, 3, 5, P, P, 0.8, 0.5, ODD, P, None, P, P, None), EINVAL),
    ("lsr_mask_nms_select", (P, P, 5, 3, 5, P, P, 0.8, 0.5, P, None, None, P, P, None), EINVAL),
    ("lsr_mask_nms_select", (P, P, 5, 3, 5, P, P, 0.8, 0.5, P, P, None, None, P, None), EINVAL),
    ("lsr_mask_nms_select", (P, P, 5, 3, 5, P, P, 0.8, 0.5, P, P, None, P, None, None), EINVAL),
    ("lsr_mask_nms_select", (P, P, -1, 3, 5, P, P, 0.8, 0.5, P, P, None, P, P, None), EINVAL),
    ("lsr_mask_nms_select", (P, P, 4097, 3, 5, P, P, 0.8, 0.5, P, P, None, P, P, None), EUNSUP),
    ("lsr_mask_nms_select", (P, P, 5, 4096, 4097, P, P, 0.8, 0.5, P, P, None, P, P, None), EUNSUP),
    ("lsr_mask_nms_select", (None, None, 0, 3, 5, None, None, 0.8, 0.5, None, None, None, None, None, None), OK),
    # lsr_mask_segmaps(words[4], kept[4], masks[4], counts[4], offsets[4], H, W, index_type, out, stream)
    ("lsr_mask_segmaps", (None, P4(), I4(), I4(), I4(), 3, 5, 0, P, None), EINVAL),
    ("lsr_mask_segmaps", (P4(), P4(), I4(), I4(), I4(), 3, 5, 0, None, None), EINVAL),
    ("lsr_mask_segmaps", (P4(), P4(), I4(), I4(), I4(), 3, 5, 2, P, None), EINVAL),
    ("lsr_mask_segmaps", (P4(), P4(), I4(), I4(), I4(), 0, 5, 0, P, None), EINVAL),
    ("lsr_mask_segmaps", (P4(), P4(), I4(), I4(), I4(), 4096, 4097, 0, P, None), EUNSUP),
    ("lsr_mask_segmaps", (P4(), P4(), I4(2), I4(1), I4(), 3, 5, 0, P, None), EINVAL),       # a counted level without pointers
    ("lsr_mask_segmaps", (P4(P), P4(P), I4(2), I4(-1), I4(), 3, 5, 0, P, None), EINVAL),
    ("lsr_mask_segmaps", (P4(P), P4(P), I4(2), I4(1), I4(-1), 3, 5, 0, P, None), EINVAL),
    ("lsr_mask_segmaps", (P4(P), P4(P), I4(2), I4(4097), I4(), 3, 5, 0, P, None), EUNSUP),
    ("lsr_mask_segmaps", (P4(P), P4(P), I4(4097), I4(1), I4(), 3, 5, 0, P, None), EUNSUP),
    # lsr_mask_boxes(words, N, H, W, boxes, stream): every rejected argument is invalid
    ("lsr_mask_boxes", (None, 5, 3, 5, P, None), EINVAL),
    ("lsr_mask_boxes", (P, 5, 3, 5, None, None), EINVAL),
    ("lsr_mask_boxes", (ODD, 5, 3, 5, P, None), EINVAL),
    ("lsr_mask_boxes", (P, 4097, 3, 5, P, None), EINVAL),
    ("lsr_mask_boxes", (P, 5, 4096, 4097, P, None), EINVAL),
    ("lsr_mask_boxes", (None, 0, 0, 5, None, None), EINVAL),      # the shape before the no-op
    ("lsr_mask_boxes", (None, 0, 3, 5, None, None), OK),
    # lsr_clip_tiles(image, H, W, words, N, keep, boxes, n, S, lut, out_type, out, stream)
    ("lsr_clip_tiles", (None, 3, 5, P, 5, P, P, 4, 224, P, 2, P, None), EINVAL),
    ("lsr_clip_tiles", (P, 3, 5, None, 5, P, P, 4, 224, P, 2, P, None), EINVAL),
    ("lsr_clip_tiles", (P, 3, 5, P, 5, P, None, 4, 224, P, 2, P, None), EINVAL),
    ("lsr_clip_tiles", (P, 3, 5, P, 5, P, P, 4, 224, P, 2, None, None), EINVAL),
    ("lsr_clip_tiles", (P, 3, 5, P, 5, P, P, 4, 224, None, 2, P, None), EINVAL),    # a float form without its table
    ("lsr_clip_tiles", (P, 3, 5, P, 5, P, P, 4, 224, None, 1, P, None), EINVAL),
    ("lsr_clip_tiles", (P, 3, 5, P, 5, None, P, 6, 224, P, 2, P, None), EINVAL),    # no keep: n <= N
    ("lsr_clip_tiles", (P, 3, 5, P, 4097, P, P, 4, 224, P, 2, P, None), EINVAL),
    ("lsr_clip_tiles", (P, 3, 5, P, 5, P, P, 4097, 224, P, 2, P, None), EINVAL),
    ("lsr_clip_tiles", (P, 3, 5, P, 5, P, P, -1, 224, P, 2, P, None), EINVAL),
    ("lsr_clip_tiles", (P, 4096, 4097, P, 5, P, P, 4, 224, P, 2, P, None), EINVAL),
    ("lsr_clip_tiles", (P, 3, 5, P, 5, P, P, 4, 0, P, 2, P, None), EINVAL),
    ("lsr_clip_tiles", (P, 3, 5, P, 5, P, P, 4, 1025, P, 2, P, None), EINVAL),
    ("lsr_clip_tiles", (P, 3, 5, P, 5, P, P, 4, 224, P, 3, P, None), EINVAL),
    ("lsr_clip_tiles", (P, 3, 5, ODD, 5, P, P, 4, 224, P, 2, P, None), EINVAL),
    ("lsr_clip_tiles", (P, 3, 5, P, 5, P, P, 4, 224, P, 1, P + 2, None), EINVAL),   # fp32 tiles on a 2-B boundary
    ("lsr_clip_tiles", (None, 0, 5, None, 5, None, None, 0, 224, None, 2, None, None), EINVAL),   # the shape first
    ("lsr_clip_tiles", (None, 3, 5, None, 5, None, None, 0, 224, None, 2, None, None), OK),
]
for fn, args, want in TABLE:
    rc = getattr(lib, fn)(*args)
    assert rc == want, (fn, args, rc, want)
    calls += 1
# the plan sizes: 0 for a shape the kernels do not take
for args, some in [((3, 64, 512, 1, 1), True), ((3, 64, 512, 64, 0), True), ((3, 32, 512, 1, 1), False),
                   ((3, 64, 17, 1, 1), False), ((3, 64, 0, 1, 1), False), ((-1, 64, 512, 1, 1), False),
                   ((3, 64, 512, 0, 1), False), ((3, 64, 512, 1, -1), False), ((3, 64, 512, 33, 32), False)]:
    assert (lib.lsr_quick_query_plan_bytes(*args) > 0) == some, args
    calls += 1
for args, some in [((3, 64, 512, 1, 0), True), ((3, 64, 512, 252, 4), True), ((3, 32, 512, 5, 4), False),
                   ((3, 64, 17, 5, 4), False), ((3, 64, 512, 0, 4), False), ((3, 64, 512, 253, 4), False),
                   ((-1, 64, 512, 5, 4), False)]:
    assert (lib.lsr_quick_semantic_plan_bytes(*args) > 0) == some, args
    calls += 1
for args, some in [((3, 64, 512, 1, 0), True), ((1, 64, 16, 60, 4), True), ((4, 64, 512, 1, 1), False),
                   ((3, 32, 512, 1, 1), False), ((3, 64, 500, 1, 1), False), ((3, 64, 512, 61, 4), False),
                   ((3, 64, 512, 0, 1), False)]:
    assert (lib.lsr_quick_heat_plan_bytes(*args) > 0) == some, args
    calls += 1
for args, some in [((3, 64, 512, 0), True), ((-1, 64, 512, 1), False), ((3, 64, 24, 1), False), ((3, 128, 512, 1), False)]:
    assert (lib.lsr_quick_decode_plan_bytes(*args) > 0) == some, args
    calls += 1
for args, some in [((1000, 64, 512), True), ((0, 1, 4), True), ((10, 0, 512), False), ((10, 257, 512), False),
                   ((10, 64, 6), False), ((10, 64, 1028), False), ((-1, 64, 512), False), ((1 << 31, 64, 512), False)]:
    assert (lib.lsr_kmeans_workspace_bytes(*args) > 0) == some, args
    calls += 1
for n, some in [(1, True), (0, True), (4096, True), (-1, False), (4097, False)]:
    assert (lib.lsr_mask_nms_workspace_bytes(n) > 0) == some, n
    calls += 1
for args, some in [((2, 4, 4), True), ((0, 4, 4), False), ((2, 0, 4), False), ((-1, 4, 4), False), ((70000, 4, 4), False)]:
    assert (lib.lsr_query_post_workspace_bytes(*args) > 0) == some, args
    calls += 1
# the render driver past validate(): missing outputs, and the empty scene's backward (a no-op)
for okw, skw, ikw, want in [(dict(out_color=P, out_lang=P, radii=None), {}, {}, EINVAL),
                            (dict(out_color=P, out_lang=None, radii=P), dict(include_feature=1),
                             dict(lang_dim=16, language_feature_precomp=P), EINVAL),
                            (dict(out_color=P, out_lang=P, radii=P), {}, dict(max_coeffs=25), EUNSUP),
                            (dict(out_color=P, out_lang=P, radii=P), dict(sh_degree=4), dict(max_coeffs=25), EINVAL),
                            (dict(out_color=P, out_lang=P, radii=P), dict(include_feature=1),
                             dict(lang_dim=1000, language_feature_precomp=P), EUNSUP),
                            (dict(out_color=P, out_lang=P, radii=P), dict(quick_render=1, quick_layout=1),
                             dict(quick_k=4, language_feature_weights_quick=P, language_feature_indices=P), EUNSUP),
                            (dict(out_color=P, out_lang=P, radii=P), dict(quick_layout=1), {}, EINVAL)]:
    rc = lib.lsr_forward(ctypes.byref(settings(**skw)), ctypes.byref(inputs(**ikw)), ctypes.byref(L.FwdOut(**okw)),
                         ALLOC, None, None)
    assert rc == want, (okw, skw, ikw, rc)
    calls += 1
for bkw, ikw, skw, want in [({}, dict(P=0), {}, OK), (dict(radii=None), {}, {}, EINVAL),
                            (dict(radii=None), dict(P=0), {}, OK),
                            ({}, dict(lang_dim=16, language_feature_precomp=P), dict(include_feature=1), EINVAL)]:
    b = dict(geom=P, binning=P, image=P, num_rendered=0, radii=P, dL_dout_color=P, dL_dout_lang=None)
    b.update(bkw)
    rc = lib.lsr_backward(ctypes.byref(settings(**skw)), ctypes.byref(inputs(**ikw)), ctypes.byref(L.BwdIn(**b)),
                          ctypes.byref(L.BwdOut()), ALLOC, None, None)
    assert rc == want, (bkw, ikw, skw, rc)
    calls += 1
# pure host code: stage-name parsing (random strings), profiling tables, versions
names = ["preprocess", "scan_tiles", "bin_count", "scan_tile_counts", "bin_scatter", "tile_sort", "render_fwd",
         "grad_zero", "render_bwd", "preprocess_bwd", "det_bounds", "det_finish"]
for _ in range(2000):
    parts = [rng.choice(names + ["", "x", "render", "render_bwdx", "a" * rng.randint(0, 300)]) for _ in
             range(rng.randint(0, 6))]
    s = ",".join(parts)
    rc = lib.lsr_profile_stages(s.encode())
    segs = s.split(",")
    if len(segs) > 1 and segs[-1] == "":
        segs = segs[:-1]   # a trailing comma is accepted
    ok = all(p in names for p in segs) if s else True
    assert (rc == 0) == ok, (s, rc)
    calls += 1
lib.lsr_profile_stages(None)
lib.lsr_profile_enable(1)
lib.lsr_profile_reset()
nm = (ctypes.c_char_p * 16)()
ms = (ctypes.c_double * 16)()
cl = (ctypes.c_int64 * 16)()
for k in (0, 1, 5, 10, 16):
    n = lib.lsr_profile_query(nm, ms, cl, k)
    assert n == min(k, len(names)), (k, n)
    calls += 1
lib.lsr_profile_enable(0)
# process-wide options: valid modes round-trip, anything else is rejected
lib.lsr_set_option.argtypes = [ctypes.c_int, ctypes.c_int64]
lib.lsr_get_option.argtypes = [ctypes.c_int, ctypes.c_void_p]
v = ctypes.c_int64(-1)
for mode in (1, 0):
    assert lib.lsr_set_option(1, mode) == 0
    assert lib.lsr_get_option(1, ctypes.byref(v)) == 0 and v.value == mode
    calls += 2
for mb in (0, 4096, 2048):   # LSR_OPT_LISTS_MAX_MB
    assert lib.lsr_set_option(2, mb) == 0
    assert lib.lsr_get_option(2, ctypes.byref(v)) == 0 and v.value == mb
    calls += 2
for on in (1, 0):             # LSR_OPT_DETERMINISTIC
    assert lib.lsr_set_option(4, on) == 0
    assert lib.lsr_get_option(4, ctypes.byref(v)) == 0 and v.value == on
    calls += 2
for opt, val in ((1, 2), (1, 3), (1, -1), (2, -5), (0, 0), (77, 1), (4, 2), (4, -1)):
    assert lib.lsr_set_option(opt, val) != 0
    calls += 1
assert lib.lsr_get_option(1, None) != 0
for code in range(-3, 10):
    assert lib.lsr_strerror(code)
    calls += 1
assert lib.lsr_abi_version() >= 6 and lib.lsr_max_lang_dim() == 64
print("ok", calls)
