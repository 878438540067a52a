"""oracle/golden_fixtures.py -- TEST INFRASTRUCTURE ONLY.  Which recipe writes which fixture: every tests/golden/*.npz belongs to exactly one runnable generator
(`python oracle/<generator> [OUT]`).  tests/test_golden_recipes.py runs each generator against the imported reference and requires the files it writes to equal
the committed ones byte for byte; a fixture that no row claims, or that two rows claim, fails that test."""

FIXTURES = {
    "gen_golden.py": [  # with its libraries gen_golden_algo.py and gen_golden_agent57.py
        "per_trace_small_nodup", "per_trace_small_dup", "per_trace_rainbow_cap3000", "per_trace_speedtest_cap4096", "per_trace_mp_cap1024",
        "per_trace_dupupdate_cap257", "per_is_kat", "functions", "target_q_n3_double", "target_q_n3_single", "target_q_n3_double_rescale_inv",
        "target_q_n5_double_h09", "target_q_n2_single_inv", "train_step_rainbow", "dqn_target_double", "dqn_target_single_rescale", "dqn_target_double_rescale",
        "rollout_items_terminated", "rollout_items_truncated", "ngu_episodic", "ngu_lifelong", "agent57_ucb", "agent57_light_target_double",
        "agent57_light_target_single_inv", "agent57_light_target_double_rescale_inv", "train_step_agent57_light", "agent57_target_s5_double",
        "agent57_target_s9_single_inv_h095", "agent57_target_s4_double_rescale_inv", "agent57_target_s1_double", "rollout_items_agent57", "train_step_agent57",
        "rankbased_trace", "rankbased_linear_trace", "episode_buffer_trace",
    ],
    "gen_golden_uniform.py": ["uniform_replay_trace"],
    "gen_golden_f1.py": ["f1_memory_plain_items", "f1_memory_compressed_items", "f1_parameter_dqn"],
    "gen_golden_actor_priority.py": ["actor_priority_n3", "actor_priority_n1"],
    "gen_golden_ppo.py": ["ppo_v_step_discrete", "ppo_v_step_continuous"],
    "gen_golden_qnet84.py": ["qnet84_init", "qnet84_wide"],
    "gen_golden_train84.py": ["train_step_rainbow84"],
    "gen_golden_agent57_84.py": ["train_step_agent57_light84"],
    "gen_golden_dqn84.py": ["train_step_dqn84"],
    "gen_golden_dqn_vec.py": ["train_step_dqn_vec"],
    "gen_golden_rainbow_vec.py": ["train_step_rainbow_vec"],
    "gen_golden_rainbow_noisy_vec.py": ["train_step_rainbow_noisy_vec"],
}
