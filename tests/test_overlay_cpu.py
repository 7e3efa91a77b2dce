"""Drawing without a GPU: the C entry point's declaration / export / descriptor layout / argument checks, the NumPy restatement's own
known answers (tests/overlay_ref.py is what the GPU tests compare detr_hip_overlay with, so it is pinned here first), the score digit
rule against "%.2f", the built-in font, palette and colormap, and draw_detections' argument validation."""
import ctypes
import os
import re

import numpy as np
import pytest

import abi_header
import overlay_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


_lib = abi_header.hip_lib


# ---- the C entry point ---------------------------------------------------------------------------------------------------------
def test_overlay_symbol_declared_exported_appended():
    _hip, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "detr_hip.h")).read()
    declared = set(re.findall(r"\b(detr_hip_[a-z0-9_]+)\s*\(", hdr))
    for name in ("detr_hip_overlay", "detr_hip_workspace_bytes_overlay"):
        assert name in declared and name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _hip.ABI_VERSION == 9 and lib.detr_hip_abi_version() == 9 and "#define DETR_HIP_ABI_VERSION 9" in hdr
    assert hdr.index("detr_overlay_desc;") > hdr.index("detr_hip_tile_merge(")          # appended, behind the newest entry
    for macro, value in (("MAX_SCALE", _hip.OVERLAY_MAX_SCALE), ("MAX_GLYPH", _hip.OVERLAY_MAX_GLYPH), ("MAX_NAME", _hip.OVERLAY_MAX_NAME),
                         ("MAX_SIDE", _hip.OVERLAY_MAX_SIDE), ("MAX_THICKNESS", _hip.OVERLAY_MAX_THICKNESS)):
        assert f"#define DETR_OVERLAY_{macro} {value}" in hdr
    assert sorted(_hip.OVERLAY_BAD) == [int(re.search(r"#define DETR_OVERLAY_BAD_COUNT (\d+)", hdr).group(1))]
    mk = open(os.path.join(ROOT, "detr-tensorflow_amd", "Makefile")).read()
    assert "csrc/overlay.hip" in mk and "build/overlay.o: EXTRA = -ffp-contract=off" in mk and "build_asan/overlay.o: EXTRA = -ffp-contract=off" in mk


def test_overlay_desc_layout_matches_the_header():
    _hip, lib = _lib()
    assert abi_header.header_structs()["detr_overlay_desc"] == list(_hip.OverlayDesc._fields_)     # names, order and types of the C declaration
    assert {w: S for w, S in _hip.LAYOUT_STRUCTS.items() if 100 <= w <= 300} == {100: _hip.DetectDesc, 200: _hip.TileMergeDesc, 300: _hip.OverlayDesc}
    assert sorted(w for w in _hip.LAYOUT_STRUCTS if w < 100) == list(range(10))
    _hip.check_struct_layouts(lib)                     # the load-time check covers it; library, unknown ids, drift: test_abi_layout_cpu.py


def test_overlay_rejects_bad_arguments_without_a_gpu():
    _hip, lib = _lib()
    fake = 4096                                   # never dereferenced: every call below fails its checks first
    required = ("src", "src_off", "dst", "dst_off", "sizes", "boxes", "labels", "counts", "colors", "atlas", "scale", "workspace", "status")
    heat = ("heat", "map_step", "map_valid", "map_scale", "lut")
    sizes = np.array([[96, 128], [1, 1]], np.int32)

    def desc(**kw):
        d = _hip.OverlayDesc()
        d.B, d.D = 2, 100
        for n in required + ("scores", "names", "name_len"):
            setattr(d, n, fake)
        d.sizes_host = sizes.ctypes.data
        d.thickness, d.label_alpha, d.fill_alpha, d.heat_alpha = 2, 255, 0, 160
        d.n_colors, d.n_names, d.name_cap, d.n_glyph, d.gh, d.gw = 100, 92, 16, 95, 8, 6
        d.glyph_digit0, d.glyph_colon, d.glyph_dot = 16, 26, 14
        d.workspace_bytes = 1 << 20
        for n, v in kw.items():
            setattr(d, n, v)
        return d

    def rejected(d, text):
        rc = lib.detr_hip_overlay(ctypes.byref(d) if d is not None else None, None)
        msg = lib.detr_hip_last_error().decode()
        assert rc < 0 and text in msg, (rc, msg, text)

    need = lib.detr_hip_workspace_bytes_overlay(ctypes.byref(desc()))
    assert need == 256 + (2 * 100 * 48 + 255) // 256 * 256 + 2 * 100 * 24             # counts | commands | text rows of name_cap + 5 -> 24 bytes
    assert lib.detr_hip_workspace_bytes_overlay(ctypes.byref(_hip.OverlayDesc())) < 0 and lib.detr_hip_workspace_bytes_overlay(None) < 0
    rejected(None, "null descriptor")
    for n in required + ("sizes_host",):
        rejected(desc(**{n: None}), "null operand")
    for kw in (dict(B=0), dict(B=-1), dict(B=65536), dict(D=0), dict(D=_hip.TILE_MAX_CAND + 1)):
        rejected(desc(**kw), "bad shape")
        assert lib.detr_hip_workspace_bytes_overlay(ctypes.byref(desc(**kw))) < 0
    for v in (0, -1, _hip.OVERLAY_MAX_THICKNESS + 1):
        rejected(desc(thickness=v), "thickness")
    for name in ("label_alpha", "fill_alpha", "heat_alpha"):
        for v in (-1, 256):
            rejected(desc(**{name: v}), name)
    rejected(desc(n_colors=0), "n_colors")
    for kw in (dict(gw=0), dict(gh=0), dict(gw=_hip.OVERLAY_MAX_GLYPH + 1), dict(gh=-2), dict(n_glyph=0)):
        rejected(desc(**kw), "bad font")
    for v in (0, -1, _hip.OVERLAY_MAX_NAME + 1):
        rejected(desc(name_cap=v), "name_cap")
    for kw in (dict(glyph_digit0=247), dict(glyph_colon=256), dict(glyph_dot=-1)):
        rejected(desc(**kw), "must fit a byte")
    for kw in (dict(n_names=-1), dict(names=None), dict(name_len=None)):
        rejected(desc(**kw), "n_names")
    for bad in ([[0, 128], [1, 1]], [[96, 128], [1, -4]], [[96, _hip.OVERLAY_MAX_SIDE + 1], [1, 1]]):
        arr = np.array(bad, np.int32)
        rejected(desc(sizes_host=arr.ctypes.data), "each side")
    for some in (heat[:1], heat[1:], heat[:4]):                                    # heat arguments: all or none
        rejected(desc(**{n: fake for n in some}), "given together")
    rejected(desc(**{n: fake for n in heat}), "bad heat map")                      # all given, Hf = Wf = 0
    rejected(desc(**{n: fake for n in heat}, Hf=3, Wf=3, sH_x=-1), "bad heat map")
    rejected(desc(workspace_bytes=need - 1), "workspace of")
    rejected(desc(workspace=fake + 4), "16-byte aligned")
    rejected(desc(boxes=fake + 8), "16-byte aligned")


# ---- the restatement's own known answers ---------------------------------------------------------------------------------------------
def test_restatement_one_box_on_an_8x8_frame():
    img = np.full((8, 8, 3), 10, np.uint8)
    colors = np.array([[200, 100, 50]], np.uint8)
    atlas = np.zeros((1, 1, 1), np.uint8)
    out = R.draw_image(img, [[1.9, 2.2, 6.5, 5.99]], [0], None, names=[], colors=colors, atlas=atlas, glyphs=(0, 0, 0), thickness=1)
    want = np.array([[0, 0, 0, 0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0],
                     [0, 1, 1, 1, 1, 1, 1, 0],                     # x from floor(1.9) = 1 to floor(6.5) = 6, y from 2 to 5
                     [0, 1, 0, 0, 0, 0, 1, 0],
                     [0, 1, 0, 0, 0, 0, 1, 0],
                     [0, 1, 1, 1, 1, 1, 1, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0]], bool)
    assert ((out == colors[0]).all(-1) == want).all() and (out[~want] == 10).all()
    # thickness 2: the 6 x 4 box is as thin as 2 t in y: all outline; a tint shows only under a thinner outline
    out = R.draw_image(img, [[1.9, 2.2, 6.5, 5.99]], [0], None, names=[], colors=colors, atlas=atlas, glyphs=(0, 0, 0), thickness=2)
    assert ((out == colors[0]).all(-1) == (want | (np.cumsum(want, 1) % 2 == 1) & want.any(1)[:, None])).all()
    out = R.draw_image(img, [[1.9, 2.2, 6.5, 5.99]], [0], None, names=[], colors=colors, atlas=atlas, glyphs=(0, 0, 0), thickness=1, fill_alpha=128)
    inner = (np.array([200, 100, 50]) * 128 + 10 * 127 + 127) // 255
    assert inner.tolist() == [105, 55, 30] and (out[3:5, 2:6] == inner).all() and (out[2, 1] == colors[0]).all()
    # skipped boxes leave the frame alone
    for box, label in (([3, 3, 2, 5], 0), ([1, 5, 4, 4], 0), ([np.nan, 1, 2, 2], 0), ([1, 1, np.inf, 2], 0), ([1, 1, 4, 4], -1)):
        assert (R.draw_image(img, [box], [label], None, names=[], colors=colors, atlas=atlas, glyphs=(0, 0, 0)) == img).all()
    # a box outside the image is clamped onto its border, as the rule says
    out = R.draw_image(img, [[-9, -9, -3, 30]], [0], None, names=[], colors=colors, atlas=atlas, glyphs=(0, 0, 0))
    assert (out[:, 0] == colors[0]).all() and (out[:, 1:] == 10).all()


def test_restatement_one_glyph_label():
    img = np.zeros((12, 12, 3), np.uint8)
    colors = np.array([[255, 255, 0], [0, 0, 90]], np.uint8)        # bright: black text; dark: white text
    atlas = np.array([[[1, 0], [0, 7], [9, 9]]], np.uint8)           # one glyph, gh = 3, gw = 2; any non-zero value is ink
    out = R.draw_image(img, [[2, 1, 11, 11]], [0], None, names=[[0]], colors=colors, atlas=atlas, glyphs=(0, 0, 0), thickness=1, scale=1,
                       label_alpha=255)
    # pad = t + s = 2: the label is 1 * 2 + 4 = 6 wide, 3 + 4 = 7 high at (2, 1); the text origin is (4, 3)
    lab = np.zeros((12, 12), bool)
    lab[1:8, 2:8] = True
    ink = np.zeros((12, 12), bool)
    ink[3, 4] = ink[4, 5] = ink[5, 4] = ink[5, 5] = True
    outline = np.zeros((12, 12), bool)
    outline[1:12, 2:12] = True
    outline[2:11, 3:11] = False
    assert ((out == 0).all(-1) == (~(lab | outline) | ink)).all()          # black: untouched background and the ink
    assert (out[(lab | outline) & ~ink] == colors[0]).all()
    # scale 2 on the dark colour: every font pixel a 2 x 2 block, white; label_alpha 0 leaves the background under the text
    out = R.draw_image(img + 40, [[0, 0, 11, 11]], [1], None, names=[[], [0]], colors=colors, atlas=atlas, glyphs=(0, 0, 0), thickness=1, scale=2,
                       label_alpha=0)
    ink2 = np.kron(atlas[0] != 0, np.ones((2, 2), bool))
    region = out[3:9, 3:7]                                                 # pad = 3
    assert (region[ink2] == 255).all() and (region[~ink2] == 40).all() and (out[1:3, 1:11] == 40).all()
    # name:score -- the text is the name, ':' and d.dd; here only its length is read off the label's width (gw * n + 2 pad)
    font = np.ones((30, 1, 1), np.uint8)
    out = R.draw_image(np.zeros((9, 40, 3), np.uint8), [[0, 0, 39, 8]], [0], [F(0.5)], names=[[1, 2]], colors=colors, atlas=font, glyphs=(10, 20, 21),
                       thickness=1, scale=1, label_alpha=255)
    assert (out[2, :12] == colors[0]).all(-1).tolist() == [True, True] + [False] * 7 + [True, True, False]        # 2 + 1 + 4 glyphs of ink


def test_score_digits_agree_with_percent_2f():
    for k in range(0, 9995):                                               # every k / 1000 below the clamp
        s = F(k / 1000)
        assert R.score_digits_rint(s) == "%.2f" % float(s) == R.score_text(s), k
    for s in (0.125, 0.375, 0.625, 0.875, 0.995, 1.0, 0.0, 9.99):
        s = F(s)
        assert R.score_digits_rint(s) == "%.2f" % float(s) == R.score_text(s), s
    assert [R.score_digits_rint(F(s)) for s in (0.125, 0.375, 0.625, 0.875)] == ["0.12", "0.38", "0.62", "0.88"]       # exact ties: half to even
    assert float(F(0.995)) > 0.995 and R.score_digits_rint(F(0.995)) == "1.00" and R.score_digits_rint(F(1.0)) == "1.00"   # 0.995f lies above 0.995
    rng = np.random.default_rng(0)
    for s in rng.random(100000).astype(F):
        assert R.score_digits_rint(s) == "%.2f" % float(s)
    for s, text in ((np.nan, "0.00"), (-0.5, "0.00"), (-0.0, "0.00"), (9.995, "9.99"), (1e9, "9.99"), (np.inf, "9.99")):
        assert R.score_digits_rint(F(s)) == R.score_text(F(s)) == text


# ---- font, palette, colormap, scale ----------------------------------------------------------------------------------------------------
def test_builtin_font():
    from detr_tf import overlay as O
    atlas = O.font_atlas()
    assert atlas.shape == (95, 8, 6) and atlas.dtype == np.uint8 and set(np.unique(atlas)) == {0, 1}
    assert atlas[0].sum() == 0                                              # the space
    assert atlas[:, 7, :].sum() == 0 and atlas[:, :, 5].sum() == 0          # 5 x 7 dots in the 6 x 8 cell
    alnum = [ord(c) - 32 for c in "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"]
    shapes = [atlas[g].tobytes() for g in alnum]
    assert all(atlas[g].sum() >= 5 for g in alnum) and len(set(shapes)) == len(shapes)
    assert len({atlas[g].tobytes() for g in range(95)}) == 95               # in fact every glyph differs
    assert O.encode_text("a:1") == [65, 26, 17] and O.encode_text("é\n~") == [31, 31, 94]          # others become '?'
    assert (atlas[ord("T") - 32][:, :5] == np.array([[1, 1, 1, 1, 1]] + [[0, 0, 1, 0, 0]] * 6 + [[0] * 5])).all()


def test_palette_colormap_and_scale_rule():
    from detr_tf import overlay as O
    p = O.class_palette(100)
    assert p.shape == (100, 3) and p.dtype == np.uint8 and (p == O.class_palette(100)).all() and (O.class_palette(7) == p[:7]).all()
    assert len({tuple(c) for c in p.tolist()}) == 100 and (p.max(1) >= 200).all()
    assert p[0].tolist() == [255, 85, 0]                                    # hue 20, full saturation and value
    with pytest.raises(ValueError):
        O.class_palette(0)
    lut = O.heat_colormap()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert lut[0].tolist() == [0, 0, 128] and lut[128].tolist() == [128, 255, 128] and lut[255].tolist() == [132, 0, 0]
    assert len({tuple(c) for c in lut.tolist()}) == 256
    for h, s in ((1, 1), (249, 1), (250, 1), (749, 1), (750, 2), (1080, 2), (1250, 3), (2160, 4)):
        assert O.default_scale(h) == s == max(1, (h + 250) // 500)
    step, valid = O.heat_geometry([[2.0, 85 / 32]], [(96, 128)], 3, 3)
    assert step.dtype == F and step.tolist() == [[F(2.0 / 96), F(85 / 32 / 128)]] and valid.tolist() == [[2, 3]]
    with pytest.raises(ValueError):
        O.heat_geometry([[0.0, 1.0]], [(96, 128)], 3, 3)


# ---- draw_detections' arguments (all checked before anything touches the device) ---------------------------------------------------
def test_draw_detections_argument_errors():
    from detr_tf.inference import Detections, Detector, draw_detections, numpy_bbox_to_image
    from detr_tf import overlay as O
    assert draw_detections is O.draw_detections and numpy_bbox_to_image is O.numpy_bbox_to_image
    img = np.zeros((20, 30, 3), np.uint8)
    ok = (np.array([[1, 1, 5, 5]], F), np.array([0]), None)
    for bad in (np.zeros((20, 30, 3), F), np.zeros((20, 30), np.uint8), np.zeros((20, 30, 4), np.uint8), [], "frame"):
        with pytest.raises(TypeError):
            draw_detections(bad if isinstance(bad, (list, str)) else [bad], [ok])
    with pytest.raises(ValueError, match="each side"):
        draw_detections([np.zeros((0, 30, 3), np.uint8)], [ok])
    for dets in ([ok, ok], [], "boxes", [np.zeros((1, 4), F)], [(ok[0], ok[1])], [{"boxes": ok[0]}]):
        with pytest.raises(ValueError):
            draw_detections([img], dets)
    with pytest.raises(ValueError, match="some images"):
        draw_detections([img, img], [ok, (ok[0], ok[1], np.array([0.5], F))])
    with pytest.raises(ValueError, match="1 boxes, 2 labels"):
        draw_detections([img], [(ok[0], np.array([0, 1]), None)])
    with pytest.raises(ValueError, match=r"\[k, 4\]"):
        draw_detections([img], [(np.zeros((2, 3), F), np.array([0, 1]), None)])
    with pytest.raises(ValueError, match="2049"):
        draw_detections([img], [(np.zeros((2049, 4), F), np.zeros(2049, np.int64), None)])
    for kw in (dict(thickness=0), dict(thickness=5000), dict(label_alpha=256), dict(fill_alpha=-1), dict(heat_alpha=300), dict(scale=0),
               dict(scale=65), dict(scale=[1, 2]), dict(colors=np.zeros((0, 3), np.uint8)), dict(colors=np.zeros((4, 3), F)),
               dict(colors=np.zeros((4, 4), np.uint8))):
        with pytest.raises(ValueError):
            draw_detections([img], [ok], **kw)

    class _Cfg:
        background_class = 91
        image_size = (64, 96)
        normalized_method = "torch_resnet"
    det = Detector(None, _Cfg(), bbox_format="xywh")
    with pytest.raises(ValueError, match="xyxy"):
        det.draw([img], [Detections(*[None] * 4)], [])
    with pytest.raises(ValueError, match="last call"):
        Detector(None, _Cfg()).draw(None, [Detections(*[None] * 4)], [])
    with pytest.raises(NotImplementedError, match="tiles"):
        Detector(None, _Cfg(), tiles=(2, 2), shortest_side=64, max_size=96).draw([img], [Detections(*[None] * 4)], [], maps={})
    cfg = _Cfg()
    cfg.normalized_method = "tf_resnet"
    with pytest.raises(ValueError, match="tf_resnet"):
        numpy_bbox_to_image(np.zeros((20, 30, 3), F), np.zeros((1, 4), F), class_name=["a"], config=cfg)
