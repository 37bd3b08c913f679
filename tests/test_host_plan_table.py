"""The planning queries (workspace bytes, statistics layout, `*_supported`) answer for every geometry of the sweep what
tests/golden/plan_table.json records -- the answers of the library before the kernel choice moved into ConvPlan / DcnPlan
(tests/golden/make_plan_table.py wrote it from that build).  Pure host code: no GPU.  One child process per environment,
since the CNUDA_* switches are read once per process.  Equality is exact."""
import json

import pytest

import make_plan_table as mpt


@pytest.fixture(scope='module')
def table():
    with open(mpt.TABLE) as f:
        return json.load(f)


def test_the_sweep_is_the_recorded_one(table):
    conv, cat, dcn = mpt.cases()
    assert table['cases'] == {'conv': conv, 'cat': cat, 'dcn': dcn}
    assert sorted(table['envs']) == sorted(mpt.ENVS)
    assert len(conv) >= 300 and len(cat) >= 20 and len(dcn) >= 60
    for env in mpt.ENVS:
        for kind in ('conv', 'cat', 'dcn'):
            assert len(table['envs'][env][kind]) == len(table['cases'][kind]), (env, kind)


@pytest.mark.parametrize('env', sorted(mpt.ENVS))
def test_planning_queries_answer_as_recorded(table, env):
    got, want = mpt.sweep_in_child(env), table['envs'][env]
    bad = []
    for kind in ('conv', 'cat', 'dcn'):
        assert len(got[kind]) == len(want[kind]), (env, kind)
        for case, g, w in zip(table['cases'][kind], got[kind], want[kind]):
            if g != w:
                bad.append((kind, case, 'got', g, 'recorded', w))
    assert not bad, '%d of the rows differ under %s; the first: %r' % (len(bad), env, bad[:5])
