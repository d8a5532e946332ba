"""-m gpu: which op each mode of SceneSession / SceneBatch launches.  The other scene tests prove bits; this one proves the path, which is
what keeps the speed where it is (profiles/scene_batch.md: the listed lift at one row is about 20 us slower than the plain one, so a
session must not drift onto the batch's ops, nor the batch onto one launch per scene).  The public lift and mean functions of ops are
wrapped with counters; the table of expected launches is written out below, call by call."""
import collections
import inspect

import pytest
import torch

from test_gpu_scene_window import _family
from test_gpu_scene_batch import _scene_metas

pytestmark = pytest.mark.gpu

LIFTS_AND_MEANS = ('backproject_mean', 'backproject_sum', 'backproject_accum_', 'backproject_gather_mean', 'backproject_gather_mean_',
                   'backproject_lists_accum_', 'backproject_lists_mean_', 'backproject_weighted_accum_', 'backproject_weighted_mean_',
                   'volume_mean', 'volume_wmean', 'volume_normalize_')


@pytest.fixture(scope='module')
def z():
    import imvoxelnet_amd
    from imvoxelnet_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), 'gpu tests need a HIP device'
    return _family(imvoxelnet_amd, 'indoor')


class _Log(list):
    def take(self):
        """{op: times called} since the last take()."""
        seen = dict(collections.Counter(name for name, _ in self))
        self.clear()
        return seen


@pytest.fixture
def log(monkeypatch):
    """Every public lift / mean of ops appends (name, its bound arguments) here, then runs."""
    from imvoxelnet_amd import ops
    calls = _Log()

    def counted(name, fn):
        sig = inspect.signature(fn)

        def wrapper(*a, **kw):
            calls.append((name, sig.bind(*a, **kw).arguments))
            return fn(*a, **kw)
        return wrapper

    for name in LIFTS_AND_MEANS:
        monkeypatch.setattr(ops, name, counted(name, getattr(ops, name)))
    return calls


def _add(s, z, views, **kw):
    return s.add_views(z['img'][torch.tensor(views, device='cuda')].contiguous(), [z['E'][v] for v in views], **kw)


def test_plain_session(z, log):
    s = z['model'].open_scene(z['scene_meta'])
    _add(s, z, [0, 1])
    assert log.take() == {'backproject_accum_': 1}
    s.volume()
    assert log.take() == {}, 'an emitting add leaves the mean ready'
    _add(s, z, [2], emit=False)
    assert log.take() == {'backproject_accum_': 1}
    s.volume()
    assert log.take() == {'volume_mean': 1}
    s.volume()
    s.detect()
    assert log.take() == {}
    s.close()


def test_fading_session(z, log):
    s = z['model'].open_scene(z['scene_meta'], decay=0.5)
    _add(s, z, [0, 1], weights=[1.0, 0.5])
    (name, args), = log
    assert name == 'backproject_weighted_accum_' and [list(l) for l in args['lists']] == [[0, 1]] and list(args['rows']) == [0]
    log.take()
    _add(s, z, [2], emit=False)
    (name, args), = log
    assert name == 'backproject_weighted_accum_' and [list(l) for l in args['lists']] == [[0]] and list(args['rows']) == [0]
    log.take()
    s.volume()
    assert log.take() == {'volume_wmean': 1}
    s.volume()
    assert log.take() == {}
    s.close()


def test_windowed_session_without_weights(z, log):
    s = z['model'].open_scene(z['scene_meta'], window=2)
    _add(s, z, [0, 1])
    assert log.take() == {}, 'a windowed add lifts nothing'
    s.volume()
    assert log.take() == {'backproject_gather_mean_': 1}
    s.volume()
    s.detect()
    assert log.take() == {}
    _add(s, z, [2])                                       # the window slides: stale again, still no weight
    s.remove_views(s.view_ids[0])
    assert log.take() == {}
    s.volume()
    assert log.take() == {'backproject_gather_mean_': 1}
    s.close()


@pytest.mark.parametrize('how', ['weights', 'reweight'])
def test_windowed_session_once_a_weight_exists(z, log, how):
    s = z['model'].open_scene(z['scene_meta'], window=3)
    if how == 'weights':
        _add(s, z, [0, 1], weights=[1.0, 0.25])
    else:
        _add(s, z, [0, 1])
        s.volume()
        assert log.take() == {'backproject_gather_mean_': 1}
        s.reweight([1], [0.25])
    assert log.take() == {}
    s.volume()
    assert log.take() == {'backproject_weighted_mean_': 1}
    s.volume()
    assert log.take() == {}
    _add(s, z, [2])                                       # no weight in this call: the scene stays on the weighted lift
    s.volume()
    assert log.take() == {'backproject_weighted_mean_': 1}
    s.close()


def test_plain_batch(z, log):
    b = z['model'].open_scenes(_scene_metas(z))
    b.add_views(z['img'][:1].contiguous(), z['E'][:1], [1])                    # touches one scene
    assert log.take() == {'backproject_lists_accum_': 1}
    b.add_views(z['img'][1:4].contiguous(), z['E'][1:4], [0, 2, 0])            # touches two
    assert log.take() == {'backproject_lists_accum_': 1}
    b.detect()
    assert log.take() == {}, 'emitting adds leave the means ready'
    b.add_views(z['img'][3:5].contiguous(), z['E'][3:5], [2, 0], emit=False)
    assert log.take() == {'backproject_lists_accum_': 1}
    b.volume(0)
    assert log.take() == {'volume_mean': 1}, 'one mean per stale scene asked for: scene 2 was not asked'
    b.detect()
    assert log.take() == {'volume_mean': 1}, 'scene 2 only: scene 0 is fresh, scene 1 was not touched'
    b.add_views(z['img'][:2].contiguous(), z['E'][:2], [0, 2], emit=False)
    b.detect([2, 0])
    assert log.take() == {'backproject_lists_accum_': 1, 'volume_mean': 2}
    b.detect()
    assert log.take() == {}
    b.close()


def test_fading_batch(z, log):
    b = z['model'].open_scenes(_scene_metas(z), decay=[1.0, 0.5, 0.75])
    b.add_views(z['img'][:3].contiguous(), z['E'][:3], [2, 0, 2], weights=[1.0, 0.5, 2.0])
    (name, args), = log
    assert name == 'backproject_weighted_accum_' and list(args['rows']) == [0, 2] and [list(l) for l in args['lists']] == [[1], [0, 2]]
    log.take()
    b.add_views(z['img'][3:4].contiguous(), z['E'][3:4], [2], emit=False)
    assert log.take() == {'backproject_weighted_accum_': 1}
    b.detect()
    assert log.take() == {'volume_wmean': 1}
    b.close()


def test_windowed_batch(z, log):
    b = z['model'].open_scenes(_scene_metas(z), window=2)
    b.add_views(z['img'][:3].contiguous(), z['E'][:3], [0, 2, 0])
    assert log.take() == {}, 'a windowed add lifts nothing'
    b.detect()
    (name, args), = log
    assert name == 'backproject_lists_mean_' and list(args['rows']) == [0, 2]
    log.take()
    b.detect()
    assert log.take() == {}
    b.add_views(z['img'][3:4].contiguous(), z['E'][3:4], [1])
    b.detect()
    (name, args), = log
    assert name == 'backproject_lists_mean_' and list(args['rows']) == [1], 'the stale scenes only'
    log.take()
    b.add_views(z['img'][4:5].contiguous(), z['E'][4:5], [2], weights=[0.5])   # the first weight: the weighted re-lift from here on
    assert log.take() == {}
    b.detect()
    (name, args), = log
    assert name == 'backproject_weighted_mean_' and list(args['rows']) == [2]
    log.take()
    b.reweight(0, [0], [0.25])
    b.volume(0)
    assert log.take() == {'backproject_weighted_mean_': 1}
    b.detect()
    assert log.take() == {}
    b.close()
