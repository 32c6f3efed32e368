"""write_pair_records -> K3MDataLoader round trip (the collation runs on the GPU, so the test is a GPU one): the
pair dicts are bit-equal to K3MPreprocessBatch.prepare + PairCollator on the records themselves, whose collation
tests/test_gpu_finetune.py checks against the reference's (golden_ft_data)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_pair_records_round_trip(dev, tmp_path):
    """six raw product TSV rows with synthetic regions -> three labelled pairs, in batches of two (the last one
    short)"""
    from k3m_amd import data as D
    from k3m_amd.loaders import CharTokenizer, K3MDataLoader, PairRecordDir, read_raw_tsv, write_pair_records
    from vilbert_k3m.datasets import K3MDataLoader as exported
    assert exported is K3MDataLoader
    rows = []
    for i in range(6):
        pv = "#;#".join("p%d%d#:#v%d%d" % (i, j, j, i) for j in range(3 + i))
        rows.append("%d\titem title %d with words\thttp://img/%d.jpg\t%s\tcat" % (1000 + i, i, i, pv))
    (tmp_path / "rows.tsv").write_text("\n".join(rows) + "\n", encoding="utf-8")
    recs = read_raw_tsv(str(tmp_path / "rows.tsv"), synthetic_regions=5)
    assert len(recs) == 6
    pairs = [(float(i % 2), recs[2 * i], recs[2 * i + 1]) for i in range(3)]
    path = str(tmp_path / "pairs")
    write_pair_records(path, pairs)
    assert sorted(os.listdir(path)) == ["item_1", "item_2", "label.npy"]
    rd = PairRecordDir(path)
    assert len(rd) == 3 and len(rd[0]) == 21 and rd[1][0] == 1.0
    kw = dict(max_seq_len=36, max_seq_len_pv=128, max_num_pv=20, max_region_len=36)
    tok = CharTokenizer()
    loader = K3MDataLoader(path, "", tok, batch_size=2, device=dev, shuffle=False, **kw)
    assert len(loader) == 2 and loader.num_dataset == 3
    got = list(loader)
    pre = D.K3MPreprocessBatch(tok, **kw)
    col = D.PairCollator(dev, 36, 2048, 1601)
    rows = [(p[0],) + tuple(p[1]) + tuple(p[2]) for p in pairs]
    for b, sl in enumerate((slice(0, 2), slice(2, 3))):
        want, ids1, ids2 = col([pre.prepare(r) for r in rows[sl]])
        want = dict(want, item_ids_1=ids1, item_ids_2=ids2)
        torch.cuda.synchronize()
        _same(got[b], want)
        assert got[b]["image_feat_1"].shape[1:] == (37, 2048) and got[b]["input_ids_pv_2"].shape[1] == 128
    assert got[0]["item_ids_1"] == [recs[0][0], recs[2][0]] and got[1]["item_ids_2"] == [recs[5][0]]
    assert got[0]["labels"].tolist() == [0.0, 1.0]
    # the same rows handed over directly, shuffled by seed: every pair once
    seen = [i for p in K3MDataLoader(None, None, tok, batch_size=2, device=dev, records=rows, seed=3, **kw)
            for i in p["item_ids_1"]]
    assert sorted(seen) == sorted(r[1] for r in rows)
    with pytest.raises(NotImplementedError):
        K3MDataLoader(str(tmp_path), "nothing_here", tok, device=dev)


def test_round_trip_matches_the_reference_collation(dev, tmp_path):
    """The six pairs of golden_ft_data (rows of the reference's bundled TSV with seeded regions, recorded with the
    reference's K3MPreprocessBatch and K3MDataLoader collation): through write_pair_records and K3MDataLoader the
    batch is bit-equal to the reference's recorded collation, and to K3MPreprocessBatch.__call__ on the rows."""
    from k3m_amd import data as D
    from k3m_amd.loaders import K3MDataLoader, write_pair_records
    from tests.test_data import char_tokenizer, ft_preprocessor, ft_records
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_ft_data.npz"))
    g = {k: z[k] for k in z.files}
    rows = ft_records(g)
    assert len(rows) == 6
    F, Ct, R = int(g["cfg/v_feature_size"]), int(g["cfg/v_target_size"]), int(g["cfg/max_region_len"])
    path = str(tmp_path / "pairs")
    write_pair_records(path, [(r[0], r[1:11], r[11:21]) for r in rows], max_boxes=R, v_feature_size=F,
                       v_target_size=Ct)
    loader = K3MDataLoader(path, "", char_tokenizer(), max_seq_len=int(g["cfg/max_seq_len"]),
                           max_seq_len_pv=int(g["cfg/max_seq_len_pv"]), max_num_pv=int(g["cfg/max_num_pv"]),
                           max_region_len=R, v_feature_size=F, v_target_size=Ct, batch_size=6, device=dev,
                           shuffle=False)
    (out,) = list(loader)
    torch.cuda.synchronize()
    assert np.array_equal(out["labels"].cpu().numpy(), g["out/labels"])
    assert out["item_ids_1"] == [str(x) for x in g["in/item_id_1"]]
    assert out["item_ids_2"] == [str(x) for x in g["in/item_id_2"]]
    pre = ft_preprocessor(g)
    tuples = [pre(r) for r in rows]   # K3MPreprocessBatch.__call__: the reference's 29-tuple per pair
    for k in (1, 2):
        assert np.array_equal(out["image_feat_%d" % k].cpu().numpy(), g["out/coll_image_feat_%d" % k], equal_nan=True)
        assert np.array_equal(out["image_loc_%d" % k].cpu().numpy(), g["out/coll_image_loc_%d" % k])
        assert np.array_equal(out["image_attention_mask_%d" % k].cpu().numpy(), g["out/coll_image_mask_%d" % k])
        for a, b in (("input_ids", "input_ids"), ("attention_mask", "input_mask"), ("token_type_ids", "segment_ids"),
                     ("input_ids_pv", "input_ids_pv"), ("attention_mask_pv", "input_mask_pv"),
                     ("token_type_ids_pv", "segment_ids_pv"), ("index_p", "index_p"), ("index_v", "index_v"),
                     ("image_target", "image_target")):
            got = out["%s_%d" % (a, k)].cpu().numpy()
            assert np.array_equal(got, g["out/%s_%d" % (b, k)]), (a, k)
            j = D.PAIR_TUPLE.index("%s_%d" % (b, k))
            assert np.array_equal(got, np.stack([t[j] for t in tuples])), (a, k)
