"""--torso_dtype: the opt-in bf16 conv path of the shallow learner.  Defaults
and refusals of the flag, and the host-side form function."""

import pytest

from scalable_agent_amd import flags as flags_lib
from scalable_agent_amd.models import Agent
from scalable_agent_amd.ops import conv


def test_default_is_auto():
  assert flags_lib.parse_flags([]).torso_dtype == 'auto'
  assert Agent(9).torso_dtype == 'auto'


def test_shallow_bf16_parses():
  f = flags_lib.parse_flags(['--torso=shallow', '--torso_dtype=bf16'])
  assert (f.torso_dtype, f.dtype) == ('bf16', 'fp32')


@pytest.mark.parametrize('argv,msg', [
    (['--torso=deep'], '--torso_dtype bf16 --torso deep'),
    (['--backend=torch'], '--torso_dtype bf16 --backend torch'),
    (['--dtype=bf16', '--backend=torch'], '--torso_dtype bf16 --dtype bf16'),
    (['--dtype=bf16', '--torso=deep'], '--torso_dtype bf16 --dtype bf16'),
])
def test_refusals(argv, msg):
  with pytest.raises(SystemExit) as e:
    flags_lib.parse_flags(['--torso_dtype=bf16'] + argv)
  assert msg in str(e.value)


def test_dtype_bf16_shallow_keeps_its_refusal():
  for extra in ([], ['--torso_dtype=bf16']):
    with pytest.raises(SystemExit) as e:
      flags_lib.parse_flags(['--dtype=bf16', '--torso=shallow'] + extra)
    assert 'the shallow torso has no bf16 HIP kernels' in str(e.value)


@pytest.mark.parametrize('shape,want', [
    ((72, 96, 3), True), ((84, 84, 4), True), ((72, 128, 1), True),
    ((72, 96, 5), False), ((72, 96, 16), False), ((64, 64, 3), False)])
def test_train_form_and_agent(shape, want):
  assert conv.shallow_bf16_train_form(shape) is want
  with pytest.raises(ValueError):
    Agent(9, frame_shape=shape, torso_dtype='fp16')
  a = Agent(9, frame_shape=shape, backend='hip', torso_dtype='bf16')
  assert a.shallow_torso_bf16_train() is want
  assert not a.shallow_torso_bf16_train(cuda=False)
  assert not Agent(9, frame_shape=shape, backend='hip').shallow_torso_bf16_train()
