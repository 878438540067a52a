"""Built-in algorithm plugins, registered under the reference's names ("QL", "DQN:torch", "Rainbow:torch",
"Rainbow_no_multisteps:torch", "Agent57_light:torch", "Agent57:torch"; "PPO:torch" and "C51:torch" stand in for the reference's
TensorFlow PPO and C51) so that a config written for the reference resolves to these classes."""
from . import agent57, agent57_light, c51, dqn, ppo, ql, rainbow  # noqa: F401
