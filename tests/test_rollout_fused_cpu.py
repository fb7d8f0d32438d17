"""unreal_maze_policy_rollout_step_encode / unreal_maze_wall_templates refuse what is outside their scope before any launch
(host checks only: no device is touched, the pointers are never followed)."""
import pytest

EINVAL = -22
P = 0x10000            # a 16-byte aligned non-null "device pointer"


@pytest.fixture(scope="module")
def built():
    from unreal_amd.build import build_library
    return build_library(verbose=False)


def _args(**over):
    """A call that passes every host check, as a dict of the prototype's arguments in order."""
    names = ("B H1 X ldx Wp bp Wv bv u pi_out v_out actions_out pos last_action last_reward count frames r_reward r_action "
             "r_terminal r_last_action r_last_reward r_pc out_reward out_terminal episode_reward score_out score_valid active "
             "active_log_t n_steps terminal_end next_idx next_lar lar_ld lar_col0 A idx_base_actor view N cfg actor_base goal "
             "layout ep_steps episode heading templates n_templates frame_scale W1 b1 W2 b2 c1_out f2_out relu_bits f2_absmax "
             "c1_absmax prepared").split()
    a = dict((n, P) for n in names)
    a.update(B=16, H1=7, ldx=264, lar_ld=264, lar_col0=256, A=4, idx_base_actor=0, view=0, N=7, cfg=None, actor_base=0,
             goal=None, layout=None, ep_steps=None, episode=None, heading=None, n_templates=1, frame_scale=1.0)
    a.update(over)
    return [a[n] for n in names] + [None]


@pytest.mark.parametrize("over", [
    dict(view=1), dict(view=2), dict(A=6), dict(A=3), dict(N=12), dict(n_templates=2), dict(templates=None),
    dict(templates=P + 8), dict(prepared=None), dict(prepared=P + 4), dict(c1_out=None), dict(relu_bits=None),
    dict(f2_out=None), dict(B=0), dict(H1=1), dict(frames=P + 1), dict(X=None), dict(ldx=255), dict(u=None),
    dict(active=None), dict(lar_ld=260), dict(r_pc=None), dict(score_out=None),
    dict(cfg=P, N=9, goal=P, layout=P, ep_steps=P, episode=P), dict(cfg=P, N=7, goal=P, layout=None, ep_steps=P, episode=P),
    dict(cfg=P, N=7, goal=P, layout=P, ep_steps=P, episode=P, n_templates=0),
])
def test_step_encode_refuses_bad_arguments(built, over):
    from unreal_amd import _lib
    L = _lib.lib()
    assert len(L.protos["unreal_maze_policy_rollout_step_encode"]) == len(_args())
    assert L._fn["unreal_maze_policy_rollout_step_encode"](*_args(**over)) == EINVAL


def test_wall_templates_refuses_bad_arguments(built):
    from unreal_amd import _lib
    f = _lib.lib()._fn["unreal_maze_wall_templates"]
    for args in ((7, None, 1, None), (7, None, 1, P + 4), (7, None, 2, P), (12, None, 1, P), (9, P, 1, P), (7, P, 0, P)):
        assert f(*args, None) == EINVAL, args
