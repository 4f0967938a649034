"""The C-ABI boundary: libmq_learner.so loads on CPU and exports every symbol include/mq_learner.h declares; the
ctypes structs match the C layout (checked by compiling a probe against the header with gcc); argument
validation errors surface as the reference's exception types without touching the GPU."""
import ctypes
import os
import re
import subprocess

import pytest

from pymarl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = [os.path.join(ROOT, "include", h) for h in ("mq_learner.h", "mc_coma.h")]


A2C_HEADER = os.path.join(ROOT, "include", "ma_a2c.h")
# every ctypes.Structure _lib defines, under the C name of its class (MQConfig: mq_config, MAPpo: ma_ppo)
STRUCTS = {c.__name__[:2].lower() + "_" + c.__name__[2:].lower(): c for c in vars(_lib).values()
           if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure}
CONSTANTS = {"MA_P_COUNT": "MA_P_COUNT", "MA_NTAIL": "MA_NTAIL", "MA_NSTATS": "MA_NSTATS", "MQ_INLINE_IDS": "INLINE_IDS",
             "MQ_PER_MAX_LIVE": "PER_MAX_LIVE", "MQ_HYPERNET_EMBED_MAX": "HYPERNET_EMBED_MAX",
             "MQ_COMM_ID_BYTES": "COMM_ID_BYTES"}


def declared_functions(headers=HEADERS):
    text = "".join(open(h).read() for h in headers)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(m[qca]_\w+)\s*\(", text, flags=re.M)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    decl = declared_functions()
    assert len(decl) >= 23
    for name in decl:
        assert hasattr(lib, name), name
    assert sorted(_lib.EXPORTS) == decl


def test_ctypes_struct_layout_matches_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "mc_coma.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(mq_config), offsetof(mq_config, gamma), offsetof(mq_config, max_seq),
         offsetof(mq_config, huber_delta), sizeof(mq_replay), offsetof(mq_replay, batch_size));
  printf("%d %d\\n", MQ_P_COUNT, MQ_NSUMS);
  printf("%zu %zu %zu %d %d %d\\n", sizeof(mc_config), offsetof(mc_config, gamma), offsetof(mc_config, max_seq),
         MC_P_COUNT, MC_NTAIL, MC_NSTATS);
  printf("%zu %zu %zu %zu\\n", sizeof(mq_plan), offsetof(mq_plan, inline_ids), offsetof(mq_plan, mix),
         offsetof(mq_plan, dwh));
  return 0;
}
""")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    c = [int(x) for x in out]
    py = [ctypes.sizeof(_lib.MQConfig), _lib.MQConfig.gamma.offset, _lib.MQConfig.max_seq.offset,
          _lib.MQConfig.huber_delta.offset,
          ctypes.sizeof(_lib.MQReplay), _lib.MQReplay.batch_size.offset, _lib.P_COUNT, _lib.NSUMS,
          ctypes.sizeof(_lib.MCConfig), _lib.MCConfig.gamma.offset, _lib.MCConfig.max_seq.offset, _lib.MC_P_COUNT,
          _lib.MC_NTAIL, _lib.MC_NSTATS, ctypes.sizeof(_lib.MQPlan), _lib.MQPlan.inline_ids.offset,
          _lib.MQPlan.mix.offset, _lib.MQPlan.dwh.offset]
    assert c == py


def test_a2c_header_declares_its_exports():
    lib = _lib.load()
    decl = declared_functions([A2C_HEADER])
    assert decl == sorted(_lib.MA_EXPORTS)
    assert declared_functions(HEADERS + [A2C_HEADER]) == sorted(_lib.EXPORTS + _lib.MA_EXPORTS)
    for name in decl:
        assert hasattr(lib, name), name


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """{name: value} from a probe the host compiler builds against the three headers: sizeof and every field offset
    of every struct in STRUCTS (the fields come from the _fields_ lists), and the constants in CONSTANTS."""
    lines = ['printf("{} %lld\\n", (long long){});'.format(c, c) for c in CONSTANTS]
    for cname, cls in STRUCTS.items():
        lines.append('printf("sizeof({0}) %zu\\n", sizeof({0}));'.format(cname))
        lines += ['printf("{0}.{1} %zu\\n", offsetof({0}, {1}));'.format(cname, f) for f, _ in cls._fields_]
    tmp = tmp_path_factory.mktemp("layout")
    src, exe = tmp / "probe.c", tmp / "probe"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mc_coma.h"\n#include "ma_a2c.h"\n'
                   "int main(void) {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.splitlines())}


def test_every_struct_is_probed():
    assert set(STRUCTS) >= {"mq_config", "mq_replay", "mq_plan", "mq_per", "mq_adam", "mc_config", "ma_config",
                            "ma_adam", "ma_ppo", "ma_plan"}


@pytest.mark.parametrize("cname", sorted(STRUCTS))
def test_struct_size_and_every_field_offset(c_layout, cname):
    cls = STRUCTS[cname]
    assert ctypes.sizeof(cls) == c_layout["sizeof({})".format(cname)]
    for f, _ in cls._fields_:
        assert getattr(cls, f).offset == c_layout["{}.{}".format(cname, f)], f


@pytest.mark.parametrize("cname", sorted(CONSTANTS))
def test_mirrored_constant(c_layout, cname):
    assert getattr(_lib, CONSTANTS[cname]) == c_layout[cname]


def test_unknown_mixer_is_value_error_before_any_hip_call():
    lib = _lib.load()
    cfg = _lib.MQConfig(n_agents=3, n_actions=9, obs_dim=30, state_dim=48, rnn_hidden_dim=64, mixing_embed_dim=32,
                        mixer=7, max_batch=4, max_seq=11)
    h = ctypes.c_void_p()
    rc = lib.mq_create(ctypes.byref(cfg), ctypes.byref(h))
    assert rc == 1
    with pytest.raises(ValueError, match="not recognised"):
        _lib.check(rc)


def test_config_validation():
    lib = _lib.load()
    h = ctypes.c_void_p()
    bad = _lib.MQConfig(n_agents=3, n_actions=9, obs_dim=30, state_dim=48, rnn_hidden_dim=32, mixing_embed_dim=32,
                        mixer=2, max_batch=4, max_seq=11)
    assert lib.mq_create(ctypes.byref(bad), ctypes.byref(h)) == 1
    assert b"rnn_hidden_dim" in lib.mq_last_error()


def test_train_without_handle_bound_reports_state_error():
    lib = _lib.load()
    assert lib.mq_apply(None, None) != 0
    assert lib.mq_forward_backward(None, None, None) != 0
    assert lib.mq_train_step(None, None, None) != 0
    assert lib.mq_last_plan(None, ctypes.byref(_lib.MQPlan())) != 0


def test_coma_host_only_entry_points():
    """COMA entry points that need no GPU: the critic-path query before any handle, the standalone critic
    forward's workspace size (coma.py:61-70 input width, include/mc_coma.h), and its argument checks."""
    lib = _lib.load()
    assert lib.mc_last_critic_path(None) == -1
    n, A, O, S = 10, 18, 176, 322
    cfg = _lib.MCConfig(n_agents=n, n_actions=A, obs_dim=O, state_dim=S, rnn_hidden_dim=64, obs_last_action=1,
                        obs_agent_id=1, max_batch=8, max_seq=181)
    B, Tq = 8, 181
    ws = lib.mc_critic_forward_workspace(ctypes.byref(cfg), B, Tq)
    Kc = S + O + 2 * n * A + n
    M = Tq * B * n
    assert ws >= M * ((Kc + 3) // 4 * 4) + 2 * M * 128 + M * A
    assert lib.mc_critic_forward_workspace(ctypes.byref(cfg), 0, Tq) == -1
    assert lib.mc_critic_forward(None, ctypes.byref(cfg), None, 0, None, None, None) != 0
    assert b"NULL" in lib.mq_last_error()
