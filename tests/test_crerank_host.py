"""CPU: the host half of the device rerank of the character-oriented mode -- cfeatures.build_rerank_tables against the two dicts of
SearchEngine.__init__ (search.py: path -> {tag: True}, path -> doc id; for a path on several lines the LAST line wins for both),
and the float32 image of the threshold.  No compute calls here."""
import numpy as np


def _engine_dicts(lines):
    """The two expressions of SearchEngine.__init__, restated (the engine itself needs a device)."""
    file_tag_index_dict = {l.split(",")[0]: {t: True for t in l.split(",")[1:]} for l in lines}
    filepath_docid_dict = {l.split(",")[0]: i for i, l in enumerate(lines)}
    return file_tag_index_dict, filepath_docid_dict


LINES = [
    "a.png,1girl,solo,hat",
    "b.png,1girl,,smile",                    # an empty tag
    "c.png,re:zero,1boy",                    # a tag containing ':'
    "a.png,2girls,hat,ribbon",               # a.png again with other tags: this line wins
    "d.png",                                 # no tags at all
    "e.png,",                                # only the empty tag
    "f.png,hat,hat,solo",                    # a tag twice on one line
]
PATHS = ["c.png", "a.png", "missing.png", "b.png", "a.png", "e.png", "d.png", "f.png"]      # a feature path missing from the file; a.png twice


def test_build_rerank_tables_follows_the_engine_dicts():
    from hiptagsearch.cfeatures import build_rerank_tables
    tags, docid = _engine_dicts(LINES)
    row_doc, row_tag_ptr, row_tags, vocab = build_rerank_tables(PATHS, LINES)
    assert row_doc.dtype == np.int32 and row_tag_ptr.dtype == np.int64 and row_tags.dtype == np.int32
    assert row_doc.shape == (len(PATHS),) and row_tag_ptr.shape == (len(PATHS) + 1,)
    assert row_tag_ptr[0] == 0 and row_tag_ptr[-1] == len(row_tags) and np.all(np.diff(row_tag_ptr) >= 0)
    names = {i: t for t, i in vocab.items()}
    assert len(names) == len(vocab)                                                        # ids are distinct
    for r, path in enumerate(PATHS):
        decoded = [names[i] for i in row_tags[row_tag_ptr[r]:row_tag_ptr[r + 1]]]
        if path not in tags:
            assert row_doc[r] == -1 and decoded == []
            continue
        assert row_doc[r] == docid[path], path
        assert set(decoded) == set(tags[path]), path
    # the cases this file was written for, spelled out
    assert row_doc[PATHS.index("a.png")] == 3 and row_doc[4] == 3                          # the last line of a duplicated path
    assert row_doc[PATHS.index("missing.png")] == -1
    assert "" in vocab and "re:zero" in vocab
    b = PATHS.index("b.png")
    assert vocab[""] in row_tags[row_tag_ptr[b]:row_tag_ptr[b + 1]]


def test_vocabulary_holds_every_tag_string_of_the_file():
    from hiptagsearch.cfeatures import build_rerank_tables
    _, _, _, vocab = build_rerank_tables(PATHS, LINES)
    want = {t for l in LINES for t in l.split(",")[1:]}
    assert set(vocab) == want                                                              # also the tags of the overridden first a.png line
    assert sorted(vocab.values()) == list(range(len(want)))


def test_tables_of_an_empty_tag_file_and_of_no_rows():
    from hiptagsearch.cfeatures import build_rerank_tables
    row_doc, row_tag_ptr, row_tags, vocab = build_rerank_tables(["x.png", "y.png"], [])
    assert list(row_doc) == [-1, -1] and list(row_tag_ptr) == [0, 0, 0] and len(row_tags) == 0 and vocab == {}
    row_doc, row_tag_ptr, row_tags, vocab = build_rerank_tables([], LINES)
    assert len(row_doc) == 0 and list(row_tag_ptr) == [0] and len(row_tags) == 0


def test_threshold_image_compares_like_numpy():
    """`np.float32 < threshold` as cfeatures_rerank evaluates it, against `d < T` in float32 with T = _threshold_f32(threshold)."""
    from hiptagsearch.cfeatures import _threshold_f32
    rng = np.random.default_rng(5)
    base = rng.random(200).astype(np.float32)
    cand = np.concatenate([base, np.nextafter(base, np.float32(2)), np.nextafter(base, np.float32(-1))]).astype(np.float32)
    for thr in [0.3, 0.11898340952738812, float(base[3]), float(base[3]) + 1e-12, float(base[4]) - 1e-12, 2.5, 0.0, -0.25,
                np.float64(base[5]) + 1e-12, np.float64(0.3), np.float32(0.3), 1]:
        t = _threshold_f32(thr)
        assert isinstance(t, np.float32)
        for d in cand:
            assert bool(d < thr) == bool(d < t), (thr, d)
