"""GPU: hiptagsearch.thumbs.ThumbnailWriter and contact_sheet, make_thumbnails.py and tagging.py --thumbnails, against Pillow: a thumbnail
is Image.fromarray(model input).resize((size, size), Image.BICUBIC) saved as JPEG, a contact sheet is a white canvas with every thumbnail
pasted into its cell, saved as JPEG -- byte for byte (resize, decode and encode are all Pillow-exact integer arithmetic).
"""
import hashlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import jpegenc_ref as jr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "anime-illust-image-searcher_amd")


def _model_inputs(n, S):
    return np.stack([jr.structured_image(S, S, 40 + i) if i % 2 else jr.noise_image(S, S, 40 + i) for i in range(n)])


def _pillow_thumbnail(x, size, quality):
    im = Image.fromarray(x)
    if im.size != (size, size):
        im = im.resize((size, size), Image.BICUBIC)
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=quality)
    return buf.getvalue()


def _rel(path):
    h = hashlib.sha1(path.encode("utf-8")).hexdigest()
    return "%s/%s.jpg" % (h[:2], h)


@pytest.mark.parametrize("S", [64, 96])
def test_thumbnail_writer_writes_pillows_files(tmp_path, S):
    import torch
    from hiptagsearch.thumbs import ThumbnailWriter, read_index
    images = _model_inputs(5, S)
    paths = ["pics/a b.png", "pics/猫.jpg", "c,d.png", "/abs/e.jpeg", "f"]
    want = [_pillow_thumbnail(x, 64, 80) for x in images]
    outs = {}
    for memory in ("host", "device"):
        out = tmp_path / memory
        with ThumbnailWriter(str(out), size=64, quality=80) as tw:
            # three batches: two on their way, the third waits for the first one's buffers
            tw.add(paths[:2], images[:2] if memory == "host" else torch.from_numpy(images[:2]).cuda())
            tw.add(paths[2:3], images[2:3] if memory == "host" else torch.from_numpy(images[2:3]).cuda())
            tw.add(paths[3:], images[3:] if memory == "host" else torch.from_numpy(images[3:]).cuda())
            tw.add([], images[:0])
        assert tw.count == 5
        assert (out / "thumbnails.csv").read_text(encoding="utf-8") == "".join("%s,%s\n" % (p, _rel(p)) for p in paths)
        outs[memory] = [(out / _rel(p)).read_bytes() for p in paths]
        assert outs[memory] == want
        assert read_index(str(out)) == {p: os.path.join(str(out), _rel(p)) for p in paths}
        assert sorted(os.listdir(str(out))) == sorted({_rel(p)[:2] for p in paths} | {"thumbnails.csv"})
    assert outs["host"] == outs["device"]


def test_thumbnail_writer_refusals(tmp_path):
    from hiptagsearch.thumbs import ThumbnailWriter
    for size in (48, 72, 528):
        with pytest.raises(ValueError):
            ThumbnailWriter(str(tmp_path / "x"), size=size)
    with pytest.raises(ValueError):
        ThumbnailWriter(str(tmp_path / "x"), quality=0)
    with ThumbnailWriter(str(tmp_path / "y"), size=64) as tw:
        with pytest.raises(ValueError):
            tw.add(["a"], _model_inputs(2, 64))
        with pytest.raises(ValueError):
            tw.add(["a"], np.zeros((1, 64, 48, 3), dtype=np.uint8))


def test_contact_sheet_equals_pillows_paste(tmp_path):
    from hiptagsearch.thumbs import ThumbnailWriter, contact_sheet
    images = _model_inputs(5, 64)
    paths = ["p%d.png" % i for i in range(5)]
    with ThumbnailWriter(str(tmp_path / "t"), size=64, quality=85) as tw:
        tw.add(paths, images)
    files = [str(tmp_path / "t" / _rel(p)) for p in paths]
    os.remove(files[3])                                                     # one path missing: its cell stays white
    (tmp_path / "t" / "broken.jpg").write_bytes(b"\xff\xd8 this is no image")
    for quality in (85, 60):
        canvas = Image.new("RGB", (192, 128), "white")
        for i, f in enumerate(files):
            if os.path.exists(f):
                canvas.paste(Image.open(f), ((i % 3) * 64, (i // 3) * 64))
        buf = io.BytesIO()
        canvas.save(buf, "JPEG", quality=quality)
        assert contact_sheet(files, columns=3, size=64, quality=quality) == buf.getvalue()
    # None, a file that does not decode and a thumbnail of another size are white cells too
    white = io.BytesIO()
    Image.new("RGB", (192, 64), "white").save(white, "JPEG", quality=85)
    with ThumbnailWriter(str(tmp_path / "t128"), size=128, quality=85) as tw:
        tw.add(["big"], _model_inputs(1, 128))
    assert contact_sheet([None, str(tmp_path / "t" / "broken.jpg"), str(tmp_path / "t128" / _rel("big"))], columns=3, size=64) == white.getvalue()


def test_query_writes_the_results_as_a_contact_sheet(tmp_path):
    """query.py --contact-sheet behind its argument parsing: result paths -> thumbnails.csv -> one JPEG in result order"""
    import query
    from hiptagsearch.thumbs import ThumbnailWriter
    images = _model_inputs(4, 64)
    paths = ["lib/p%d.png" % i for i in range(4)]
    with ThumbnailWriter(str(tmp_path / "t"), size=64, quality=85) as tw:
        tw.add(paths, images)
    ranked = [paths[2], "lib/not-in-the-cache.png", paths[0], paths[3], paths[1]]
    query.write_contact_sheet(ranked, str(tmp_path / "t"), str(tmp_path / "sheet.jpg"), columns=2)
    canvas = Image.new("RGB", (128, 192), "white")
    for i, p in enumerate(ranked):
        if p in paths:
            canvas.paste(Image.open(str(tmp_path / "t" / _rel(p))), ((i % 2) * 64, (i // 2) * 64))
    buf = io.BytesIO()
    canvas.save(buf, "JPEG", quality=85)
    assert (tmp_path / "sheet.jpg").read_bytes() == buf.getvalue()


def _run(script, args, cwd):
    res = subprocess.run([sys.executable, os.path.join(PKG, script)] + args, cwd=str(cwd), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    return res.stdout


_PICS = {}


def _pics(tmp_path_factory):
    """a directory of six small JPEG / PNG files (one RGBA, two not square) and one file that is no image; made once"""
    if not _PICS:
        pics = tmp_path_factory.mktemp("thumbs") / "pics"
        pics.mkdir()
        rng = np.random.default_rng(5)
        for i in range(6):
            h, w = [(80, 80), (64, 64), (100, 70), (48, 90), (64, 64), (120, 120)][i]
            a = jr.structured_image(h, w, 70 + i)
            if i == 2:
                im = Image.fromarray(np.dstack([a, rng.integers(0, 256, (h, w), dtype=np.uint8)]), "RGBA")
            else:
                im = Image.fromarray(a)
            if i % 2:
                im.save(str(pics / ("f%d.jpg" % i)), "JPEG", quality=90)
            else:
                im.save(str(pics / ("f%d.png" % i)))
        (pics / "broken.png").write_bytes(b"this is no image")
        _PICS["dir"] = str(pics)
    return _PICS["dir"]


def _check_cache(thumbs_dir, size=64, quality=85):
    """the cache lists the six decodable files (in the order the directory walk gives them), and every thumbnail is Pillow's of the tagger's
    model input; returns the paths"""
    from hiptagsearch import pipeline
    rows = [line.rsplit(",", 1) for line in (thumbs_dir / "thumbnails.csv").read_text(encoding="utf-8").splitlines()]
    assert sorted(os.path.basename(p) for p, _ in rows) == ["f0.png", "f1.jpg", "f2.png", "f3.jpg", "f4.png", "f5.jpg"]
    for path, rel in rows:
        assert rel == _rel(path)
        assert (thumbs_dir / rel).read_bytes() == _pillow_thumbnail(pipeline.decode_image(path, 64), size, quality), path
    return [p for p, _ in rows]


def test_tagging_writes_thumbnails_and_the_same_tags(tmp_path, tmp_path_factory):
    """tagging.py --model vit-tiny (a 64-pixel model input) --workers 2 with and without --thumbnails: Pillow's thumbnails, the same tag file"""
    d = _pics(tmp_path_factory)
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    plain.mkdir()
    flagged.mkdir()
    _run("tagging.py", ["--dir", d, "--model", "vit-tiny", "--workers", "2", "--batch", "4"], plain)
    _run("tagging.py", ["--dir", d, "--model", "vit-tiny", "--workers", "2", "--batch", "4", "--thumbnails", "thumbs", "--thumb-size", "64",
                        "--thumb-quality", "85"], flagged)
    tags = (plain / "tags-wd-tagger.txt").read_bytes()
    assert len(tags.splitlines()) == 6 and (flagged / "tags-wd-tagger.txt").read_bytes() == tags
    assert _check_cache(flagged / "thumbs") == [line.split(",")[0] for line in tags.decode("utf-8").splitlines()]
    assert not (plain / "thumbs").exists()


def test_tagging_refuses_thumbnails_where_no_pipeline_runs(tmp_path, tmp_path_factory):
    d = _pics(tmp_path_factory)
    for extra in (["--compat", "--workers", "2"], ["--synthetic", "4", "--workers", "2"], [], ["--workers", "2", "--thumb-size", "72"]):
        res = subprocess.run([sys.executable, os.path.join(PKG, "tagging.py"), "--dir", d, "--model", "vit-tiny", "--thumbnails", "t"] + extra,
                             cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
        assert res.returncode == 2 and "--thumb" in res.stderr, extra
        assert not (tmp_path / "t").exists() and not (tmp_path / "tags-wd-tagger.txt").exists()


@pytest.mark.parametrize("mode", [[], ["--gpu-resize", "--gpu-jpeg", "--gpu-png"]], ids=["host-decode", "device-decode"])
def test_make_thumbnails_writes_the_same_files_in_every_input_mode(tmp_path, tmp_path_factory, mode):
    """make_thumbnails.py over the same directory: what tagging.py --thumbnails writes (both are held to Pillow's bytes), whether the
    worker processes decode and resize or the device does"""
    d = _pics(tmp_path_factory)
    out = _run("make_thumbnails.py", ["--dir", d, "--out", "thumbs", "--size", "64", "--input-size", "64", "--workers", "2", "--batch", "4"] + mode,
               tmp_path)
    assert "6 thumbnails" in out
    from hiptagsearch.tagger import Predictor
    assert _check_cache(tmp_path / "thumbs") == [p for p in Predictor.list_files_recursive(None, d) if not p.endswith("broken.png")]
