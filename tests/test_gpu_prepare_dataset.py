"""scripts/prepare_dataset.py end to end on a temporary folder: file names and pixels equal what the three reference
scripts produce one after the other -- Pillow's LANCZOS resize under the multiscale rules (pinned to the scripts by
tests/test_cpu_prep.py), the numpy crop of extract_subimages.py:82-99 restated here, and the oracle's PIL-'L' + Laplacian
mask restatement that test_offline_mask_tool_writes_reference_formats uses."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import pil_resize_reference as R
from oracle import ssg_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROP, STEP, EDGE = 32, 16, 40


def _tool():
    spec = importlib.util.spec_from_file_location("prepare_dataset", os.path.join(ROOT, "scripts", "prepare_dataset.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _crops(img, name, ext):
    """extract_subimages.py:75-99 on an array."""
    name = name.replace('x2', '').replace('x3', '').replace('x4', '').replace('x8', '')
    h, w = img.shape[:2]
    h_space = np.arange(0, h - CROP + 1, STEP)
    if h - (h_space[-1] + CROP) > 0:
        h_space = np.append(h_space, h - CROP)
    w_space = np.arange(0, w - CROP + 1, STEP)
    if w - (w_space[-1] + CROP) > 0:
        w_space = np.append(w_space, w - CROP)
    out, index = {}, 0
    for x in h_space:
        for y in w_space:
            index += 1
            out[f'{name}_s{index:03d}{ext}'] = np.ascontiguousarray(img[x:x + CROP, y:y + CROP, ...])
    return out


@pytest.mark.gpu
def test_prepare_dataset_writes_what_the_reference_chain_writes(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from PIL import Image
    from ssl_amd import maskio, prep
    src, sub, masks, ms = (tmp_path / n for n in ("gt", "sub", "masks", "multiscale"))
    src.mkdir()
    sources = {"0001x2": R.content('blocks', 70, 93, 3, seed=1) // 2 + R.content('random', 70, 93, 3, seed=2) // 2,
               "grey": R.content('random', 64, 57, 1, seed=3)[..., 0],
               "low": R.content('random', 37, 80, 3, seed=4)}          # shorter side under EDGE: not kept, S upscales
    for name, a in sources.items():
        Image.fromarray(a).save(str(src / f"{name}.png"))
    tool = _tool()
    args = ["--input", str(src), "--save", str(sub), "--variant", "gan", "--shortest-edge", str(EDGE), "--crop-size",
            str(CROP), "--step", str(STEP), "--masks", str(masks), "--threshold", "20", "--keep-multiscale", str(ms)]
    assert tool.main(args) == 0

    want_ms, want_sub = {}, {}
    for name, a in sources.items():
        plan, keep = prep.multiscale_plan(a.shape[1], a.shape[0], 'gan', EDGE)
        assert keep == (name != "low")
        items = {name + suffix: np.array(Image.fromarray(a).resize(size, resample=Image.LANCZOS)) for suffix, size in plan}
        if keep:
            items[name] = a
        for stem, im in items.items():
            want_ms[stem + ".png"] = im
            want_sub.update(_crops(im, stem, ".png"))
    assert "0001T0_s001.png" in want_sub and "lowS_s001.png" in want_sub and "low_s001.png" not in want_sub
    assert sorted(os.listdir(str(ms))) == sorted(want_ms)
    for f, im in want_ms.items():
        assert np.array_equal(np.array(Image.open(str(ms / f))), im), f
    assert sorted(os.listdir(str(sub))) == sorted(want_sub)
    report = open(str(masks / "statis.txt")).read()
    assert sorted(os.listdir(str(masks / "mat"))) == sorted(f[:-4] + ".mat" for f in want_sub)
    assert sorted(os.listdir(str(masks / "png"))) == sorted(want_sub)
    for f, crop in want_sub.items():
        assert np.array_equal(np.array(Image.open(str(sub / f))), crop), f
        rgb = crop if crop.ndim == 3 else np.repeat(crop[..., None], 3, axis=2)
        want = orc.edge_mask_rgb8(rgb, 20.0)
        got = maskio.load_mask_mat(str(masks / "mat" / (f[:-4] + ".mat")))
        assert got.shape == want.shape + (1,) and np.array_equal(got[..., 0], want.astype(np.float32)), f
        assert np.array_equal(np.array(Image.open(str(masks / "png" / f))), want * 255), f
        n, ng, nm = want.size, int(orc.edge_mask_rgb8(rgb, 0.0).sum()), int(want.sum())
        assert f"{f[:-4]}:\nImage number-{n}, grad number-{ng}-{ng / n:.4f}, mask number-{nm}-{nm / n:.4f}\n" in report
    assert "Average of grad is" in report

    # without --keep-multiscale and --masks nothing but the sub-image folder is written
    only = tmp_path / "only"
    assert tool.main(["--input", str(src), "--save", str(only / "sub"), "--shortest-edge", str(EDGE), "--crop-size",
                      str(CROP), "--step", str(STEP)]) == 0
    assert os.listdir(str(only)) == ["sub"] and sorted(os.listdir(str(only / "sub"))) == sorted(want_sub)
    assert sorted(os.listdir(str(tmp_path))) == ["gt", "masks", "multiscale", "only", "sub"]
