"""The host-side queries of csrc/conv.hip (kernel class, weight format, workspace sizes, head chunks) answer what
tests/golden/conv_routes.json records for every shape x precision x operand maxima x tuning flag of
tests/golden/make_golden_conv_routes.py.  The queries read the same route functions as the dispatch, so an unintended change
of routing shows here, without a GPU (the queries never touch the device)."""
import json
import os

import make_golden_conv_routes as mk

FIELDS = (['class(%d)' % p for p in (0, 1, 2)] + ['planes(%d)' % p for p in (0, 1)] + ['wgrad_ws', 'head_chunks(K)', 'head_chunks(17)'] +
          ['fwd_bnstats_ws(G=%d)' % g for g in mk.GROUPS] + ['dgrad_bn_bwd_ws(G=%d)' % g for g in mk.GROUPS])


def test_queries_answer_the_recorded_routes():
    from xas_amd import _lib
    _lib.load()
    with open(mk.OUT) as f:
        doc = json.load(f)
    assert [tuple(s) for s in doc['shapes']] == mk.SHAPES and tuple(doc['precisions']) == mk.PRECISIONS
    assert tuple(doc['amax']) == mk.AMAX and tuple(doc['tunes']) == mk.TUNES and tuple(doc['groups']) == mk.GROUPS
    prec = _lib.query('xas_get_precision')
    got = mk.table(_lib)
    assert _lib.query('xas_get_precision') == prec
    assert len(got) == len(doc['records']) == len(mk.SHAPES) * 4 * 3 * 5
    bad = []
    for (i, p, a, t), g, want in zip(mk.cases(), got, doc['records']):
        assert len(g) == len(want) == len(FIELDS)
        bad += ['%s prec %d amax %s tune %s: %s = %d, recorded %d' % (mk.SHAPES[i], p, a, t, n, x, y)
                for n, x, y in zip(FIELDS, g, want) if x != y]
    assert not bad, '%d differences, first: %s' % (len(bad), '; '.join(bad[:8]))


def test_the_table_reaches_every_route():
    """Every kernel class for every pass, both weight formats and plane counts, epilogue and separate-pass workspaces."""
    with open(mk.OUT) as f:
        recs = json.load(f)['records']
    for col, want in ((0, {0, 1, 2, 3, 4}), (1, {0, 1, 2, 3, 4}), (2, {0, 1, 2, 3, 4}), (3, {0, 1, 2, 3}), (4, {0, 1, 2, 3})):
        assert {r[col] for r in recs} == want, FIELDS[col]
    assert {r[6] > 0 for r in recs} == {True, False}
