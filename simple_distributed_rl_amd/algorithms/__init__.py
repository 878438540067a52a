"""Built-in algorithm plugins, registered under the reference's names ("QL", "DQN:torch", "Rainbow:torch",
"Rainbow_no_multisteps:torch", "Agent57_light:torch", "Agent57:torch"; "PPO:torch", "C51:torch", "R2D2:torch" and "SAC_Discrete:torch" stand in for the
reference's TensorFlow PPO, C51, R2D2 and discrete SAC: restatements on torch/ROCm, parity unpinned, each checked against a float64 restatement under
tests/; "V-PPO:torch" and "NoT_SAC:torch" are the reference's own torch PPO and target-free SAC, pinned on it) so that a config written for the reference resolves to these classes."""
from . import agent57, agent57_light, c51, dqn, ppo, ppo_v, ql, r2d2, rainbow, sac, sac_not  # noqa: F401
