"""GPU: window renders (pt_render_window, pt_render_window_async, pt_frame_window) against the oracle.

A pixel's result depends on its coordinates in the IMAGE only (camera_ray: the seed index, the
jitter, norm_x / norm_y), never on where it sits in a launch, so a window's pixels carry the bits of
the same rectangle of the full render: every comparison here is `same_bits` against the oracle's row
band oracle.frame / oracle.render(y0, y1) cropped to the window's columns.

Shapes are the smallest at which the slot -> pixel mapping can go wrong: the image 40x24 (24x16 for
the boat) is no multiple of the 16x16 block, of a 64-path batch or of the 8x8 wave tile; window
A = (5, 3, 19, 7) is 133 paths (a ragged 64-path batch, an odd width, across block borders),
B = (13, 9, 17, 11).  A and B see light in every scene used (the oracle's lit pixels, frames 3, 7, 11
at depth 16: CornellBox 110 of 133 / 172 of 187, Glossy 66 / 181, Sphere 65 / 186, the boat's A 30),
and each parity test on them asserts ref.mean() > 0, so a black window cannot pass as equal.
"""
import functools
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
import pt_amd
from conftest import PKG, SCENES
from test_gpu_parity import ENV_KEYS, KERNELS, mismatch_report, same_bits

pytestmark = pytest.mark.gpu

W, H = 40, 24
A = (5, 3, 19, 7)
B = (13, 9, 17, 11)
DEPTH = 16
INI = os.path.join(SCENES, "scene_files", "final", "cornell_box_full_lighting.ini")
_PACKED = {}


def crop(img, win):
    x0, y0, w, h = win
    return np.ascontiguousarray(img[y0:y0 + h, x0:x0 + w])


@functools.lru_cache(maxsize=None)
def _ref_frame(scene, w, h, win, salt, depth):
    p = _PACKED[scene]
    x0, y0, ww, wh = win
    band, _ = oracle.frame(p.triangle_data, p.bvh_data, p.meta_for(w, h), salt, depth, y0=y0, y1=y0 + wh)
    out = np.ascontiguousarray(band[:, x0:x0 + ww])
    out.setflags(write=False)
    return out


def ref_frame(packed, scene, w, h, win, salt, depth=DEPTH):
    _PACKED[scene] = packed[scene]
    return _ref_frame(scene, w, h, win, salt, depth)


def ref_render(p, meta, win, frame0, nframes, stride, depth, init=None):
    """The oracle's accumulator (and counters) of the window's ROWS, cropped to its columns; init:
    the window's initial accumulator [h][w][3]."""
    x0, y0, w, h = win
    acc = np.zeros((h, int(meta[0]), 3), np.float32)
    if init is not None:
        acc[:, x0:x0 + w] = init
    band, cnt = oracle.render(p.triangle_data, p.bvh_data, meta, frame0, nframes, stride, depth, acc=acc, y0=y0, y1=y0 + h)
    return np.ascontiguousarray(band[:, x0:x0 + w]), cnt


@pytest.fixture
def defaults(ptopts):
    for k in ENV_KEYS:
        ptopts.unset(k, raising=False)
    return ptopts


@pytest.fixture(params=list(KERNELS))
def kernel(request, ptopts):
    for k in ENV_KEYS:
        ptopts.unset(k, raising=False)
    for k, v in KERNELS[request.param].items():
        ptopts.set(k, v)
    return request.param


# ---------------------------------------------------------------------------------------------
# 1. pt_frame_window over the whole variant matrix
# ---------------------------------------------------------------------------------------------
def _check_frames(packed, scene, w, h, windows, salts, label):
    p = packed[scene]
    meta = p.meta_for(w, h)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        for win in windows:
            for t in salts:
                gpu = s.frame(meta, t, DEPTH, window=win)
                ref = ref_frame(packed, scene, w, h, win, t)
                assert gpu.shape == (win[3], win[2], 3)
                assert ref.mean() > 0
                assert same_bits(gpu, ref), f"{scene} {win} t={t} {label}: " + mismatch_report(gpu, ref)


@pytest.mark.parametrize("scene", ["CornellBox", "CornellBox-Sphere"])
def test_frame_window_bitexact(packed, kernel, scene):
    """CornellBox: the fused kernel and the mailbox path; the sphere: k_wf_generate + k_wf_trace."""
    _check_frames(packed, scene, W, H, (A, B), (0, 977), kernel)


@pytest.mark.parametrize("variant", ["auto", "wavefront_lean_lds"])
def test_frame_window_boat(packed, ptopts, variant):
    for k in ENV_KEYS:
        ptopts.unset(k, raising=False)
    for k, v in KERNELS[variant].items():
        ptopts.set(k, v)
    _check_frames(packed, "MedievalBoat", 24, 16, (A,), (0, 977), variant)


# ---------------------------------------------------------------------------------------------
# 2. pt_render_window: accumulation onto a random accumulator, counted and plain builds
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [pt_amd.MODE_MEGAKERNEL, pt_amd.MODE_WAVEFRONT, pt_amd.MODE_AUTO],
                         ids=["megakernel", "wavefront", "auto"])
@pytest.mark.parametrize("scene", ["CornellBox", "CornellBox-Glossy"])
@pytest.mark.parametrize("win", [A, B], ids=["A", "B"])
def test_render_window_accum_bitexact(packed, defaults, scene, mode, win):
    """frame0 3, 3 frames, stride 4: the wavefront's batch is two parts of 2 + 1 frames."""
    p = packed[scene]
    meta = p.meta_for(W, H)
    init = np.random.default_rng(7).uniform(0, 1, (win[3], win[2], 3)).astype(np.float32)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        counted, _ = s.render(meta, 3, 3, 4, DEPTH, mode, accum=init.copy(), counters=True, window=win)
        plain = s.render(meta, 3, 3, 4, DEPTH, mode, accum=init.copy(), window=win)
    ref, _ = ref_render(p, meta, win, 3, 3, 4, DEPTH, init)
    zero, _ = ref_render(p, meta, win, 3, 3, 4, DEPTH)
    assert zero.mean() > 0
    assert same_bits(counted, ref), mismatch_report(counted, ref)
    assert same_bits(plain, ref), mismatch_report(plain, ref)


# ---------------------------------------------------------------------------------------------
# 3. counters of a full-width window == the oracle's row band's
# ---------------------------------------------------------------------------------------------
def test_window_counters_match_oracle_band(packed, defaults):
    p = packed["CornellBox"]
    meta = p.meta_for(W, H)
    win = (0, 9, W, 11)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        gpu, gc = s.render(meta, 3, 3, 4, DEPTH, pt_amd.MODE_MEGAKERNEL, counters=True, window=win)
    ref, rc = oracle.render(p.triangle_data, p.bvh_data, meta, 3, 3, 4, DEPTH, y0=9, y1=20)
    assert ref.mean() > 0
    assert same_bits(gpu, ref), mismatch_report(gpu, ref)
    assert set(gc) == {"samples", "ext_queries", "shadow_queries", "nodes", "tri_tests", "box_tests"}
    assert gc == rc, (gc, rc)
    assert gc["samples"] == W * 11 * 3


# ---------------------------------------------------------------------------------------------
# 4. identity: no window and the whole-image window are Scene.render
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [pt_amd.MODE_MEGAKERNEL, pt_amd.MODE_WAVEFRONT], ids=["megakernel", "wavefront"])
def test_full_window_is_the_plain_render(packed, defaults, mode):
    p = packed["CornellBox"]
    meta = p.meta_for(33, 17)
    lib = pt_amd.load_library()
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        plain = s.render(meta, 0, 3, 1, DEPTH, mode)
        full = s.render(meta, 0, 3, 1, DEPTH, mode, window=(0, 0, 33, 17))
        null = np.zeros((17, 33, 3), np.float32)  # pt_render_window with win = NULL
        assert lib.pt_render_window(s._h, meta.ctypes.data, None, 0, 3, 1, DEPTH, mode, null.ctypes.data, None) == 0
        fplain = s.frame(meta, 5, DEPTH)
        ffull = s.frame(meta, 5, DEPTH, window=(0, 0, 33, 17))
    ref, _ = oracle.render(p.triangle_data, p.bvh_data, meta, 0, 3, 1, DEPTH)
    assert ref.mean() > 0
    assert same_bits(plain, ref), mismatch_report(plain, ref)
    assert plain.tobytes() == full.tobytes() == null.tobytes()
    assert fplain.tobytes() == ffull.tobytes()


# ---------------------------------------------------------------------------------------------
# 5. edges
# ---------------------------------------------------------------------------------------------
EDGES = [(0, 0, 1, 1), (W - 1, H - 1, 1, 1), (0, 11, W, 1), (21, 0, 1, H), (0, 0, 8, 8), (3, 2, 13, 5)]


@pytest.mark.parametrize("win", EDGES, ids=["corner00", "cornerWH", "row", "column", "64paths", "65paths"])
@pytest.mark.parametrize("kern", ["mega", "wavefront"])
def test_window_edges(packed, defaults, win, kern):
    defaults.set("kernel", kern)
    p = packed["CornellBox"]
    meta = p.meta_for(W, H)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        gpu = s.frame(meta, 7, DEPTH, window=win)
        acc = s.render(meta, 3, 3, 4, DEPTH, window=win)
    ref = ref_frame(packed, "CornellBox", W, H, win, 7)
    racc, _ = ref_render(p, meta, win, 3, 3, 4, DEPTH)
    assert same_bits(gpu, ref), mismatch_report(gpu, ref)
    assert same_bits(acc, racc), mismatch_report(acc, racc)


# ---------------------------------------------------------------------------------------------
# 6. several batches, ragged last one; the in-kernel camera batches
# ---------------------------------------------------------------------------------------------
BATCHES = [{"wf_paths": 200}, {"parts": 3}, {"wf_paths": 200, "fuse_gen": 1}, {"parts": 3, "fuse_gen": 1},
           {"wf_paths": 200, "fuse_gen": 0}, {"parts": 3, "fuse_gen": 0},
           {"wf_paths": 200, "fuse_gen": 1, "regen": 1}, {"parts": 3, "fuse_gen": 1, "regen": 1}]


@pytest.mark.parametrize("scene", ["CornellBox", "CornellBox-Sphere"])
def test_window_several_batches(packed, defaults, scene):
    """Window A (133 paths), 5 frames: wf_paths=200 makes batches of 2 + 2 + 1 frames, parts=3 up to
    three parts; fuse_gen / regen: the fused kernel's own camera batches (CornellBox)."""
    p = packed[scene]
    meta = p.meta_for(W, H)
    ref, _ = ref_render(p, meta, A, 2, 5, 3, DEPTH)
    assert ref.mean() > 0
    got = []
    for opts in BATCHES:
        for k in ("wf_paths", "parts", "fuse_gen", "regen"):
            defaults.unset(k)
        for k, v in opts.items():
            defaults.set(k, v)
        with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
            got.append(s.render(meta, 2, 5, 3, DEPTH, pt_amd.MODE_WAVEFRONT, window=A))
        assert same_bits(got[-1], ref), f"{opts}: " + mismatch_report(got[-1], ref)
    for g in got[1:]:
        assert same_bits(g, got[0])


# ---------------------------------------------------------------------------------------------
# 7. tiling
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [(16, 16), (7, 5)])
@pytest.mark.parametrize("scene", ["CornellBox", "CornellBox-Glossy"])
def test_render_tiled_equals_full_render(packed, defaults, scene, tile):
    p = packed[scene]
    meta = p.meta_for(W, H)
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        full, fc = s.render(meta, 3, 3, 4, DEPTH, pt_amd.MODE_AUTO, counters=True)
        tiled, tc = pt_amd.render_tiled(s, meta, 3, 3, 4, DEPTH, pt_amd.MODE_AUTO, tile=tile, counters=True)
        plain = pt_amd.render_tiled(s, meta, 3, 3, 4, DEPTH, pt_amd.MODE_AUTO, tile=tile)
    assert full.mean() > 0
    assert tiled.shape == (H, W, 3)
    assert same_bits(tiled, full), mismatch_report(tiled, full)
    assert same_bits(plain, full), mismatch_report(plain, full)
    for k in ("samples", "ext_queries", "shadow_queries"):
        assert tc[k] == fc[k], (k, tc, fc)


# ---------------------------------------------------------------------------------------------
# 8. row pitch: windows rendered in place inside a full image
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [pt_amd.MODE_MEGAKERNEL, pt_amd.MODE_WAVEFRONT], ids=["megakernel", "wavefront"])
def test_window_async_row_pitch(packed, defaults, mode):
    torch = pytest.importorskip("torch")
    p = packed["CornellBox"]
    meta = p.meta_for(W, H)
    wins = (A, (24, 10, 16, 14))  # disjoint; the second touches the image's right and bottom edges
    sentinel = -12345.5
    img = torch.full((H, W, 3), sentinel, dtype=torch.float32, device="cuda")
    for x0, y0, w, h in wins:
        img[y0:y0 + h, x0:x0 + w] = 0.0
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        for win in wins:
            s.render_window_async(meta, win, 3, 3, 4, DEPTH, mode, img.data_ptr() + 12 * (win[1] * W + win[0]),
                                  row_pitch=W, stream_ptr=st.cuda_stream)
        st.synchronize()
        s.check()
        full = s.render(meta, 3, 3, 4, DEPTH, mode)
    got = img.cpu().numpy()
    outside = np.ones((H, W), bool)
    for win in wins:
        assert crop(full, win).mean() > 0
        assert same_bits(crop(got, win), crop(full, win)), f"{win}: " + mismatch_report(crop(got, win), crop(full, win))
        outside[win[1]:win[1] + win[3], win[0]:win[0] + win[2]] = False
    assert np.all(got[outside] == np.float32(sentinel))


# ---------------------------------------------------------------------------------------------
# 9. rejection
# ---------------------------------------------------------------------------------------------
def test_bad_windows_rejected_and_scene_stays_usable(packed, defaults):
    torch = pytest.importorskip("torch")
    p = packed["CornellBox"]
    meta = p.meta_for(W, H)
    buf = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    with pt_amd.Scene(p.triangle_data, p.bvh_data) as s:
        for win in ((30, 0, 11, 4), (0, 20, 4, 5), (0, 0, 0, 4), (0, 0, 4, 0), (W, 0, 1, 1), (0, H, 1, 1)):
            for call in (lambda: s.render(meta, 0, 1, 1, DEPTH, window=win),
                         lambda: s.frame(meta, 0, DEPTH, window=win),
                         lambda: s.render_async(meta, 0, 1, 1, DEPTH, pt_amd.MODE_AUTO, buf.data_ptr(), window=win,
                                                row_pitch=W)):
                with pytest.raises(pt_amd.PtError) as e:
                    call()
                assert e.value.code == -1 and "window" in str(e.value), win
        for pitch in (A[2] - 1, 0):
            with pytest.raises(pt_amd.PtError) as e:
                s.render_async(meta, 0, 1, 1, DEPTH, pt_amd.MODE_AUTO, buf.data_ptr(), window=A, row_pitch=pitch)
            assert e.value.code == -1 and "row_pitch" in str(e.value)
        with pytest.raises(pt_amd.PtError) as e:  # no window: the pitch is checked against the image's width
            s.render_async(meta, 0, 1, 1, DEPTH, pt_amd.MODE_AUTO, buf.data_ptr(), row_pitch=W - 1)
        assert e.value.code == -1
        torch.cuda.synchronize()
        assert float(buf.abs().max()) == 0.0  # nothing was rendered
        gpu = s.frame(meta, 0, DEPTH, window=A)
    ref = ref_frame(packed, "CornellBox", W, H, A, 0)
    assert ref.mean() > 0
    assert same_bits(gpu, ref), mismatch_report(gpu, ref)


# ---------------------------------------------------------------------------------------------
# 10. Node: programEntry's window option and pt-render.js --window
# ---------------------------------------------------------------------------------------------
NODE_SCRIPT = r"""
const fs = require('fs');
const host = require(process.argv[1]);
(async () => {
    const s = host.load_scene_from_ini(process.argv[2], { web_root: process.argv[3], quiet: true });
    const S = s.scene_description.Settings;
    S.imageWidth = %d; S.imageHeight = %d; S.samplesPerPixel = 3;
    const dim = host.screen_dimension(S);
    const out = process.argv[4];
    for (const mode of ['megakernel', 'wavefront']) {
        const full = await host.programEntry(dim, s.primitive_data, s.camera_data, s.scene_description, { mode });
        const win = await host.programEntry(dim, s.primitive_data, s.camera_data, s.scene_description,
                                            { mode, window: %s, chunk: 2, counters: true });
        fs.writeFileSync(`${out}/${mode}_accum.f32`, Buffer.from(full.accum.buffer));
        fs.writeFileSync(`${out}/${mode}_rgba.u8`, Buffer.from(full.rgba.buffer));
        fs.writeFileSync(`${out}/${mode}_win_accum.f32`, Buffer.from(win.accum.buffer));
        fs.writeFileSync(`${out}/${mode}_win_rgba.u8`, Buffer.from(win.rgba.buffer));
        fs.writeFileSync(`${out}/${mode}_counters.json`, JSON.stringify(win.counters));
    }
    let bad = null;
    try {
        await host.programEntry(dim, s.primitive_data, s.camera_data, s.scene_description, { window: [30, 0, 11, 4] });
    } catch (e) { bad = e.message; }
    fs.writeFileSync(out + '/bad.json', JSON.stringify({ bad }));
})().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
""" % (W, H, json.dumps(list(A)))


def test_node_program_entry_window():
    with tempfile.TemporaryDirectory() as td:
        subprocess.run(["node", "-e", NODE_SCRIPT, os.path.join(PKG, "node"), INI, SCENES, td], check=True,
                       capture_output=True, timeout=300)
        for mode in ("megakernel", "wavefront"):
            acc = np.fromfile(os.path.join(td, mode + "_accum.f32"), np.float32).reshape(H, W, 3)
            rgba = np.fromfile(os.path.join(td, mode + "_rgba.u8"), np.uint8).reshape(H, W, 4)
            wacc = np.fromfile(os.path.join(td, mode + "_win_accum.f32"), np.float32).reshape(A[3], A[2], 3)
            wrgba = np.fromfile(os.path.join(td, mode + "_win_rgba.u8"), np.uint8).reshape(A[3], A[2], 4)
            cnt = json.load(open(os.path.join(td, mode + "_counters.json")))
            assert crop(acc, A).mean() > 0
            assert wacc.tobytes() == crop(acc, A).tobytes()
            assert np.array_equal(wrgba, crop(rgba, A))
            assert cnt["samples"] == A[2] * A[3] * 3
        bad = json.load(open(os.path.join(td, "bad.json")))["bad"]
    assert bad and "pt_hip error -1" in bad and "window" in bad


def test_pt_render_cli_window_png():
    from PIL import Image
    cli = ["node", os.path.join(PKG, "node", "bin", "pt-render.js"), INI, "--web-root", SCENES, "--spp", "2",
           "--max-depth", "4"]
    win = (200, 40, 19, 7)  # under the light of the .ini's own image
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run(cli + ["--out-root", os.path.join(td, "full")], check=True, capture_output=True, text=True,
                           timeout=300)
        full_info = json.loads(r.stdout.strip().splitlines()[-1])
        full = np.array(Image.open(full_info["output"]))
        r = subprocess.run(cli + ["--out-root", os.path.join(td, "win"), "--window", ",".join(map(str, win))], check=True,
                           capture_output=True, text=True, timeout=300)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        img = np.array(Image.open(info["output"]))
    assert (info["width"], info["height"], info["window"]) == (19, 7, list(win))
    assert img.shape == (7, 19, 4)
    assert full.shape[0] >= win[1] + win[3] and full.shape[1] >= win[0] + win[2]
    assert np.array_equal(img, crop(full, win))
    assert img[..., :3].max() > 0
