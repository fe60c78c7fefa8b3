"""Batch conventions checked against what the reference's own helpers (caption_src/data_io.py:
get_sub_frames, collate_fn, custom_dset_train / custom_dset_test, filt_word_category) return on the same inputs -- recorded
in tests/golden/data_io.npz by tools/gen_golden.py --data-io-only -- and against hand-worked layouts.  CPU only."""
import os

import numpy as np
import pytest
import torch

from controllable_xgating_amd.data import CaptionDataset, collate, get_sub_frames, make_video_item, word_categories

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_io.npz")
# the inputs of the recorded reference calls (tools/gen_golden.py:gen_data_io regenerates them from here)
SUB_FRAME_LENGTHS = (5, 26, 27, 100)
ITEM_KEYS = ("id", "cap", "cap_class", "class_mask", "feat1", "feat2", "feat_mask", "pos_feat", "gts")
POS_TAGS = ("FW -LRB- -RRB- LS VB VBD VBP VBG VBN VBZ NN NNS NNP NNPS JJ JJR JJS RB RBS RBR WRR WRB EX CC PRP PRP$ WP POS WP$ IN TO "
            "DT WDT PDT RP MD CD SYM : `` # $ UH , . ''").split()


def _golden():
    with np.load(GOLDEN, allow_pickle=False) as g:
        return {k: g[k] for k in g.files}


def _items(rng):
    items = []
    for n_frames, cap in ((40, [5, 9, 3, 7]), (11, [4, 2]), (26, [8, 6, 2, 9, 11, 3])):
        f1 = rng.random((n_frames, 6)).astype(np.float32); f2 = rng.random((n_frames, 4)).astype(np.float32)
        pos = rng.random((len(cap) + 1, 5)).astype(np.float32)
        a, b, m, p = make_video_item(f1, f2, pos, 26)
        items.append(dict(cap=cap, cap_class=[c % 3 for c in cap], class_mask=[1] * len(cap), feat1=a, feat2=b, feat_mask=m,
                          pos_feat=p, raw=(f1, f2, pos)))
    return items


def test_subsample_pad_and_mask():
    rng = np.random.default_rng(0)
    long = rng.random((40, 6)).astype(np.float32)
    short = rng.random((11, 6)).astype(np.float32)
    s = get_sub_frames(long, 26)
    assert s.shape == (26, 6) and np.array_equal(s[0], long[0]) and np.array_equal(s[13], long[int(13 * 40 / 26)])
    p = get_sub_frames(short, 26)
    assert np.array_equal(p[:11], short) and not p[11:].any()
    f1, f2, mask, pos = make_video_item(short, rng.random((11, 4)).astype(np.float32), rng.random((3, 5)).astype(np.float32), 26)
    assert mask.shape == (1, 26) and mask[0, :11].all() and not mask[0, 11:].any()


def test_collate_layout():
    items = _items(np.random.default_rng(1))
    caps, caps_mask, cap_classes, class_masks, feats1, feats2, feat_mask, pos_feat = collate(items)
    assert caps.shape == (3, 7) and caps[:, 0].eq(0).all()                       # BOS column
    assert caps[0].tolist() == [0, 8, 6, 2, 9, 11, 3]                           # sorted longest first
    assert caps_mask.sum(1).tolist() == [7.0, 5.0, 3.0]                          # BOS + n words
    assert class_masks[1].tolist() == [1, 1, 1, 1, 1, 0, 0]                      # n ones + the extra 1 (data_io.py:360)
    assert feats1.shape == (3, 26, 6) and feat_mask.shape == (3, 26) and pos_feat.shape == (3, 5)


def test_against_reference_helpers():
    ref = _golden()
    rng = np.random.default_rng(2)
    for n in SUB_FRAME_LENGTHS:
        fr = rng.random((n, 8)).astype(np.float32)
        assert np.array_equal(ref["sub_frames_%d" % n], get_sub_frames(fr, 26))
    items = _items(rng)
    mine = collate(items)
    assert len(mine) == 8
    for i, b in enumerate(mine):
        assert torch.equal(torch.from_numpy(ref["collate_%d" % i]).float(), b.float())


# ------------------------------------------------------------------ on-disk side (data_io.py:51-126, :128-328)
def _corpus(rng):
    caps = {"vid1": [dict(caption="A cat runs.", tokenized="a cat runs"), dict(caption="The cat is quickly running away now", tokenized="the cat is quickly running away now"),
                     dict(caption="", tokenized="")],
            "vid2": [dict(caption="Two dogs play", tokenized="two dogs play zzz"), dict(caption="dogs", tokenized="dogs")],
            "vid3": [dict(caption="x", tokenized="and he sings")]}
    split = ["vid1_0", "vid1_1", "vid1_2", "vid2_0", "vid2_1", "vid3_0"]
    words = ["a", "cat", "runs", "the", "is", "quickly", "running", "away", "two", "dogs", "play", "and", "he", "sings"]
    worddict = {wd: i + 2 for i, wd in enumerate(words)}
    category = {"NN": ["cat"], "NNS": ["dogs"], "VBZ": ["runs", "is", "sings"], "VBG": ["running"], "DT": ["a", "the"], "RB": ["quickly", "away"],
                "CD": ["two"], "CC": ["and"], "PRP": ["he"], "VBP": ["play"], "XX": ["now"]}
    f1 = {v: rng.random((n, 6)).astype(np.float32) for v, n in (("vid1", 30), ("vid2", 7), ("vid3", 12))}
    f2 = {v: rng.random((len(f1[v]), 4)).astype(np.float32) for v in f1}
    pos = {v: {"states": rng.random((5, 8)).astype(np.float32)} for v in f1}
    return split, caps, worddict, category, f1, f2, pos


def test_word_categories_and_dataset_items():
    split, caps, worddict, category, f1, f2, pos = _corpus(np.random.default_rng(3))
    cat = word_categories(category, dict(worddict, **{"<EOS>": 0, "UNK": 1}))
    assert cat["cat"] == 3 and cat["dogs"] == 3 and cat["runs"] == 2 and cat["quickly"] == 5 and cat["two"] == 11 and cat["he"] == 7
    assert cat["<EOS>"] == 0 and cat["<UNK>"] == 1 and cat["UNK"] == 1
    ds = CaptionDataset(split, caps, worddict, category, f1, f2, pos, K=10, seq_length=6)
    assert ds.ids == ["vid1_0", "vid2_0", "vid2_1", "vid3_0"]                   # empty and 7-token captions dropped (data_io.py:158)
    it = ds[1]
    assert it["cap"] == [10, 11, 12, 1] and it["cap_class"] == [11, 3, 2, 1]     # 'zzz' is out of vocabulary -> 1 / category 1
    assert it["feat1"].shape == (10, 6) and not it["feat1"][7:].any() and it["feat_mask"].tolist() == [[1.0] * 7 + [0.0] * 3]
    assert torch.equal(it["pos_feat"], torch.from_numpy(pos["vid2"]["states"][-1]))
    assert it["gts"].tolist() == [[10, 11, 12, 1], [11, 0, 0, 0]]                # the video's references, longest first, zero padded
    assert CaptionDataset(split, caps, worddict, category, f1, f2, pos, K=10, seq_length=6, test=True).ids == ["vid1_0", "vid2_0", "vid3_0"]
    batch = collate([ds[i] for i in range(len(ds))])                             # feeds straight into the collate convention
    assert batch[0].shape == (4, 5) and batch[4].shape == (4, 10, 6)


def test_dataset_against_reference_classes():
    ref = _golden()
    split, caps, worddict, category, f1, f2, pos = _corpus(np.random.default_rng(4))
    for test, kind in ((False, "train"), (True, "test")):
        mine = CaptionDataset(split, caps, worddict, category, f1, f2, pos, K=10, seq_length=6, test=test)
        assert ref["%s_ids" % kind].tolist() == mine.ids
        for i in range(len(mine)):
            data, cap, cap_class, class_mask, a, b, m, p_, gts = (ref["%s_%d_%s" % (kind, i, k)] for k in ITEM_KEYS)
            it = mine[i]
            assert data.item() == it["id"] and cap.tolist() == it["cap"] and cap_class.tolist() == it["cap_class"] \
                and class_mask.tolist() == it["class_mask"]
            assert torch.equal(torch.from_numpy(a), it["feat1"]) and torch.equal(torch.from_numpy(b), it["feat2"]) \
                and torch.equal(torch.from_numpy(m), it["feat_mask"]) and torch.equal(torch.from_numpy(p_), it["pos_feat"])
            assert np.array_equal(gts, it["gts"])


def test_every_pos_tag_maps_like_the_reference_table():
    """caption_src/data_io.py:60-100, tag by tag -- including the reference's own 'WRR' (sic, :64; pos_src/ spells it 'WRB',
    but the training path is caption_src): a word tagged WRB is category 1 in the reference, and here."""
    ref = _golden()
    tags = POS_TAGS
    category = {t: ["w%d" % i] for i, t in enumerate(tags)}
    words = ["w%d" % i for i in range(len(tags))] + ["untagged"]
    theirs = ref["pos_tag_category"]
    assert theirs.shape == (len(tags),)
    mine = word_categories(category, words)
    for i, t in enumerate(tags):
        assert mine["w%d" % i] == int(theirs[i]), (t, mine["w%d" % i], int(theirs[i]))
    assert mine["untagged"] == int(ref["pos_untagged_category"]) == 1
    assert mine["w%d" % tags.index("WRB")] == 1 and mine["w%d" % tags.index("WRR")] == 5 and mine["w%d" % tags.index("RB")] == 5


def test_hdf5_feature_store_roundtrip(tmp_path):
    h5py = pytest.importorskip("h5py")
    if not hasattr(h5py, "File"):                 # (a stand-in module registered by other code, not the real package)
        pytest.skip("h5py is not installed")
    split, caps, worddict, category, f1, f2, pos = _corpus(np.random.default_rng(5))
    for name, store in (("rgb", f1), ("opfl", f2)):
        with h5py.File(tmp_path / (name + ".hdf5"), "w") as f:
            for v, arr in store.items():
                f[v] = arr
    with h5py.File(tmp_path / "pos.hdf5", "w") as f:
        for v, g in pos.items():
            f.create_group(v)["states"] = g["states"]
    from controllable_xgating_amd.data import open_feature_store
    ds = CaptionDataset(split, caps, worddict, category, open_feature_store(tmp_path / "rgb.hdf5"), open_feature_store(tmp_path / "opfl.hdf5"),
                        open_feature_store(tmp_path / "pos.hdf5"), K=10, seq_length=6)
    ref_ds = CaptionDataset(split, caps, worddict, category, f1, f2, pos, K=10, seq_length=6)
    for i in range(len(ds)):
        assert torch.equal(ds[i]["feat1"], ref_ds[i]["feat1"]) and torch.equal(ds[i]["pos_feat"], ref_ds[i]["pos_feat"])
