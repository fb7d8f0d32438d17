"""Minibatched reuse epochs without a GPU: option checks, the flag, the order of a reuse epoch's blocks and the
argument checks of unreal_minibatch_gather."""
import pytest
import torch


@pytest.fixture(scope="module")
def built():
    from unreal_amd.build import build_library
    return build_library(verbose=False)


def test_check_minibatch_options():
    from unreal_amd.train.trainer import Trainer
    chk = Trainer.check_minibatch_options
    for env_type in ("maze", "arcade", "lab", "gym", "indoor"):
        assert chk(env_type, 7, 1, 1) == 1                        # off: every environment, whatever the batch
    assert chk("maze", 8, 1, 2) == 2 and chk("arcade", 512, 1, 64) == 64 and chk("maze", 8, 2, 4) == 4
    assert chk("maze", 8, 8, 1) == 1 and chk("maze", 6, 2, 3) == 3
    for B, G, M in ((8, 1, 3), (8, 2, 8), (8, 2, 3), (6, 1, 4), (4, 4, 2)):
        with pytest.raises(ValueError, match="divide"):
            chk("maze", B, G, M)                                  # M does not divide Bg = B // G
    for env_type in ("lab", "gym", "indoor"):
        with pytest.raises(ValueError, match="host-fed"):
            chk(env_type, 8, 1, 2)
    for bad in (0, -1, True, False, 2.0, "2", None):
        with pytest.raises(ValueError, match="reuse_minibatches"):
            chk("maze", 8, 1, bad)
    # the three-argument check of the reuse options keeps its signature
    assert Trainer.check_reuse_options("maze", 1, 0.2) == (1, 0.2)


def test_flag_name_and_default():
    from unreal_amd.options import get_options
    f = get_options("training")
    assert f.reuse_minibatches == 1
    g = get_options("training", argv=["--reuse_minibatches", "64"])
    assert g.reuse_minibatches == 64 and isinstance(g.reuse_minibatches, int)


@pytest.mark.parametrize("M", [1, 2, 5])
def test_minibatch_order_is_a_rotating_permutation(M):
    from unreal_amd.train.trainer import Trainer
    first = Trainer.minibatch_order(1, M)
    assert first == list(range(M))
    for e in range(1, 2 * M + 3):
        order = Trainer.minibatch_order(e, M)
        assert sorted(order) == list(range(M))                    # every block once per epoch
        assert order == [(i + e - 1) % M for i in range(M)]
        nxt = Trainer.minibatch_order(e + 1, M)
        assert nxt == order[1:] + order[:1]                       # the next epoch starts one block later


def test_trainer_refuses_before_touching_the_device():
    """The constructor checks the option first: no network, no device needed."""
    from unreal_amd.train.trainer import Trainer
    args = (0, None, 7e-4, None, None, "lab", "nav_maze_static_01", True, True, True, True, 0.05, 0.001, 20, 20, 0.99, 0.9,
            2000, 10 ** 6, "cuda:0")
    with pytest.raises(ValueError, match="host-fed"):
        Trainer(*args, batch_size=8, reuse_minibatches=2)
    with pytest.raises(ValueError, match="reuse_minibatches"):
        Trainer(*args, batch_size=8, reuse_minibatches=0)
    maze = args[:5] + ("maze", "") + args[7:]
    with pytest.raises(ValueError, match="divide"):
        Trainer(*maze, batch_size=8, groups=2, reuse_minibatches=3)


def test_entry_refuses_bad_arguments_without_launch(built):
    """Fake device pointers: every call below is refused on the host, so none of them reaches a kernel."""
    from unreal_amd import _lib, ops
    L = _lib.lib()
    fn = L._fn["unreal_minibatch_gather"]
    dev = 1 << 20
    #       T  Bg Bm j0 A  frame_idx actions active adv R pi | the six outputs            | side ld  | xcat x_out c0 h0 c0_out h0_out
    good = [5, 8, 2, 6, 4, dev, dev, dev, dev, dev, dev, dev, dev, dev, dev, dev, dev, 5, 261, dev, dev, dev, dev, dev, dev]
    assert len(good) == len(L.protos["unreal_minibatch_gather"]) - 1
    ff = list(good)
    ff[17], ff[19:25] = 0, [None] * 6                             # feed-forward: none of the LSTM streams

    def with_(base=good, **kw):
        a = list(base)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return a
    bad = [with_(_0=0), with_(_0=-1),                             # T
           with_(_2=0), with_(_2=-2),                             # Bm
           with_(_3=-1), with_(_3=7), with_(_1=7),                # j0 < 0, j0 + Bm > Bg
           with_(_4=1), with_(_4=19), with_(_4=0),                # A outside 2..18
           with_(_17=-1), with_(_17=6), with_(_18=260), with_(_18=0),     # the side width is negative / does not fit in ld
           with_(ff, _17=-1), with_(ff, _18=255)]
    bad += [with_(**{"_%d" % k: None}) for k in range(5, 17)]     # required pointers
    bad += [with_(ff, **{"_%d" % k: None}) for k in range(5, 17)]
    bad += [with_(**{"_%d" % k: None}) for k in range(19, 25)]    # some but not all of the LSTM streams
    bad += [with_(ff, **{"_%d" % k: dev}) for k in range(19, 25)]
    bad += [with_(_19=None, _20=None), with_(_21=None, _22=None, _23=None, _24=None)]
    bad += [with_(**{"_%d" % k: dev + 4}) for k in range(21, 25)]  # a start-state pointer off the 16-byte grid
    for a in bad:
        assert fn(*a, None) == -22, a
    with pytest.raises(_lib.UnrealLibError):
        L.call("unreal_minibatch_gather", *with_(_0=0), None)
    x, n = torch.zeros(5 * 8 * 4), torch.zeros(5 * 8 * 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.minibatch_gather(5, 8, 2, 6, 4, n, n, n, x, x, x, n, n, n, x, x, x)
    with pytest.raises(ValueError, match="j0"):
        ops.minibatch_gather(5, 8, 2, 7, 4, n, n, n, x, x, x, n, n, n, x, x, x)
    with pytest.raises(ValueError, match="side"):
        ops.minibatch_gather(5, 8, 2, 6, 4, n, n, n, x, x, x, n, n, n, x, x, x, side=5, ld=260)
    with pytest.raises(ValueError, match="go together"):
        ops.minibatch_gather(5, 8, 2, 6, 4, n, n, n, x, x, x, n, n, n, x, x, x, side=5, ld=261, xcat=x)
