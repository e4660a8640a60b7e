#!/usr/bin/env python3
"""Plays a TocabiAMPLower AMP policy from a checkpoint, as the reference's play path does (paths relative to
python/IsaacGymEnvs/isaacgymenvs/learning): restore (amp_players.py:47-61), the text export TOCABI's controller reads
(rl_games_custom/torch_runner_dyros.py:143-149), then CommonPlayer.run's loop (common_player.py:51-149): reset_done, the policy's action, step,
the reward and the steps summed per env; on done envs `reward: ... steps: ...` (the means over the envs done at that step), at the end
`av reward: ... av steps: ...`.

The action is AmpActorCritic.play: the actor in eval mode, deterministic (clamp(mu, -1, 1); rl_games' rescale_actions is the identity on this
task's +-1 action space) unless --stochastic.  On --policy_backend hip that is dwa_play.

rl_games' player defaults are not part of the reference's checkout; the defaults here: --games 100, --max_steps 10000 (more than the 8000-step
episode, so every game can end on its own).

--report switches on the env's on-GPU episode statistics (cfg sim.mi355.amp_episode_stats, isaacgymdyros_amd/amp_episode_stats.py) and prints
their table after playing: termination causes and their combinations, contact bodies, episode lengths, reward terms, command tracking and
sole loads.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from isaacgymdyros_amd import amp_checkpoint as CK    # noqa: E402
from amp_consumer import make_env                     # noqa: E402


def run(args):
    dev = torch.device(args.device)
    env = make_env(args.num_envs, args.device, args.motion_file, args.synthetic, episode_stats=args.report)
    if args.export_dir:
        CK.export_txt(args.checkpoint, args.export_dir)
    pol, disc = CK.load_policy(args.checkpoint, dev, backend=args.policy_backend, with_disc=True)
    if (pol.D, pol.A) != (env.num_obs, env.num_actions):
        raise SystemExit("checkpoint: %d observations / %d actions, the task has %d / %d" % (pol.D, pol.A, env.num_obs, env.num_actions))
    N, games_played, sum_rewards, sum_steps = env.num_envs, 0, 0.0, 0.0
    for _ in range(args.games):
        if games_played >= args.games:
            break
        env.reset()
        cr = torch.zeros(N, device=dev)
        steps = torch.zeros(N, device=dev)
        for _n in range(args.max_steps):
            obs = env.reset_done()[0]["obs"].contiguous()
            noise = torch.randn(N, pol.A, device=dev) if args.stochastic else None
            with torch.no_grad():
                action, _mu = pol.play(obs, noise)
            _obs, r, done, info = env.step(action)
            cr += r.view(N)
            steps += 1
            if args.print_disc_prediction:
                amp = info["amp_obs"][0:1].contiguous().view(1, 1, -1)
                _c, disc_r, logit = disc.rewards(amp, torch.zeros(1, 1, 1, device=dev), return_logits=True)
                print("disc_pred: ", float(logit.view(-1)[0]), float(disc_r.view(-1)[0]))
            idx = done.nonzero(as_tuple=False).view(-1)
            k = int(idx.numel())
            if k > 0:
                games_played += k
                cur_r, cur_s = float(cr[idx].sum()), float(steps[idx].sum())
                keep = 1.0 - done.float().view(N)
                cr, steps = cr * keep, steps * keep
                sum_rewards += cur_r
                sum_steps += cur_s
                print("reward:", cur_r / k, "steps:", cur_s / k, flush=True)
                if games_played >= args.games:
                    break
    print(sum_rewards)
    if games_played == 0:
        raise SystemExit("no game ended within --max_steps %d" % args.max_steps)
    av_r, av_s = sum_rewards / games_played, sum_steps / games_played
    print("av reward:", av_r, "av steps:", av_s, flush=True)
    if args.report:
        from isaacgymdyros_amd.amp_episode_stats import format_table
        print(format_table(env.episode_stats.summary()), flush=True)
    if not (math.isfinite(av_r) and math.isfinite(av_s)):
        raise SystemExit("non-finite average")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--checkpoint", required=True, help="a checkpoint of examples/amp_consumer.py --output_dir (or the reference learner's)")
    ap.add_argument("--num_envs", type=int, default=64)
    ap.add_argument("--games", type=int, default=100)
    ap.add_argument("--max_steps", type=int, default=10000, help="steps per round of games before the envs are reset")
    ap.add_argument("--motion_file", default=None)
    ap.add_argument("--synthetic", action="store_true", help="the synthetic motion tables of tests/amp_motion_synth.py")
    ap.add_argument("--stochastic", action="store_true", help="sample mu + exp(sigma) noise instead of the deterministic mu")
    ap.add_argument("--policy_backend", default="hip", choices=["hip", "torch"])
    ap.add_argument("--print_disc_prediction", action="store_true", help="env 0's discriminator logit and reward every step")
    ap.add_argument("--export_dir", default=None, help="write the network tensors and the observation normaliser as text files here")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--report", action="store_true", help="sim.mi355.amp_episode_stats: print the episode statistics' table after playing")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
