"""GPU: find_duplicates.py as a child process on a directory of files -- the near-duplicate corpus of tests/imghash_ref.py (every
picture as a PNG, a smaller PNG and a JPEG of quality 75, plus unrelated pictures), an all-white PNG and a file that is no image.

Guard: the test first asserts the separation condition of its own corpus with the numpy restatement (copies within 10 bits, different
pictures beyond 20), so a failure further down points at the device and not at the recipe.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import imghash_ref as ir

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "anime-illust-image-searcher_amd", "find_duplicates.py")


def _run(args, cwd):
    res = subprocess.run([sys.executable, SCRIPT] + args, cwd=str(cwd), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-4000:]
    return res.stdout


def test_cli_recovers_the_planted_groups(tmp_path):
    from PIL import Image
    corpus = ir.near_duplicate_corpus(20260301, pictures=4, singles=3)           # 15 files
    H = ir.hash128(ir.corpus_inputs(corpus))
    pid = {name: p for name, p, _ in corpus}
    ir.assert_separation(H, [p for _, p, _ in corpus])                           # the guard
    assert (ir.set_bits(H) >= 8).all()
    pics = tmp_path / "pics"
    (pics / "sub").mkdir(parents=True)
    for k, (name, _, data) in enumerate(corpus):
        (pics / "sub" / name if k % 2 else pics / name).write_bytes(data)
    Image.new("RGB", (300, 200), (255, 255, 255)).save(str(pics / "white.png"))
    (pics / "broken.png").write_bytes(b"this is no image")

    out = _run(["--dir", "pics", "--workers", "2", "--batch", "8", "--save-hashes", "saved", "--out", "duplicates.csv"], tmp_path)
    text = (tmp_path / "duplicates.csv").read_text(encoding="utf-8")
    rows = [line.rsplit(",", 1) for line in text.splitlines()]
    names = [os.path.basename(p) for p, _ in rows]
    assert sorted(names) == sorted(list(pid) + ["white.png"])                    # one line per decodable file
    labels = {n: int(l) for n, (_, l) in zip(names, rows)}
    assert labels["white.png"] == -1
    groups = {}
    for n in pid:
        if pid[n] < 4:
            groups.setdefault(labels[n], set()).add(pid[n])
            assert labels[n] >= 0, n
        else:
            assert labels[n] == -1, n                                            # the singles
    assert sorted(groups) == [0, 1, 2, 3] and all(len(s) == 1 for s in groups.values())      # each group is one picture, no two share one
    # numbered by their first file in input order
    first = [labels[n] for n in names if labels[n] >= 0]
    assert [l for i, l in enumerate(first) if l not in first[:i]] == [0, 1, 2, 3]
    assert "16 files, 4 groups, 12 files in groups, 1 flat files" in out

    # the device's hashes are the restatement's, file by file (the pool decodes with Pillow, pads and resizes as tagger_input does)
    saved = np.load(str(tmp_path / "saved.npy"))
    saved_paths = (tmp_path / "saved.csv").read_text(encoding="utf-8").splitlines()
    assert saved_paths == [p for p, _ in rows] and saved.dtype == np.uint64 and saved.shape == (16, 2)
    by_name = {name: h for (name, _, _), h in zip(corpus, H)}
    for p, h in zip(saved_paths, saved):
        n = os.path.basename(p)
        assert h.tolist() == (by_name[n].tolist() if n in by_name else [0, 0]), n

    (pics / "white.png").unlink()                                                # no image is touched: the files may go
    _run(["--hashes", "saved", "--max-distance", "10", "--min-set-bits", "8", "--out", "again.csv"], tmp_path)
    assert (tmp_path / "again.csv").read_bytes() == (tmp_path / "duplicates.csv").read_bytes()
