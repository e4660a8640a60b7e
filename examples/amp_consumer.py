#!/usr/bin/env python3
"""The consumer side of TocabiAMPLower: the reference's AMP learner, restated in plain torch around the HIP discriminator
(isaacgymdyros_amd/amp_disc.py).  Paths relative to python/IsaacGymEnvs/isaacgymenvs; configured by cfg/train/TocabiAMPLowerPPO.yaml
(amp_disc.TRAIN_CFG, or --train_yaml):

  network         separate actor / critic MLPs 512-512 relu (nn.Linear's own initialisation: initializer `default`), linear mu / value heads,
                  a fixed log-sigma of sigma_init = -1.6 (`learn_sigma: False`).  sigma_last (-2.99) is NOT scheduled for this learner: the
                  only code that reads it is learning/rl_games_custom/models_dyros.py:64-70 (the DYROS walk model); amp_continuous builds
                  learning/amp_models.py's ModelAMPContinuous, whose sigma stays at its initial value.
  play_steps      learning/amp_continuous.py:91-167 -- eval mode; next values zeroed on `terminate`; amp_obs recorded; the discriminator's
                  reward over the whole rollout (ONE dwd_reward launch over horizon x envs rows), combined 0.7 task + 0.3 disc; GAE
                  (common_agent.py:413-425)
  train_epoch     :176-258 -- one demo top-up (512), a demo sample and a replay sample as large as the batch (the current batch on the first
                  epoch), 6 mini epochs over minibatches of 131072 (or the whole batch if smaller), replay store with keep probability
  calc_gradients  :260-329 -- clipped surrogate (e_clip 0.2), critic loss (critic_coef 5), bound loss (bounds_loss_coef 10, soft bound 1),
                  the discriminator's share through AmpDiscriminator.update (its own Adam at the same learning rate: Adam is per parameter,
                  so one optimiser over all parameters steps them alike; no clipping: truncate_grads False)
  normalisation   normalize_input / normalize_value (rl_games' RunningMeanStd, amp_disc.RunningMeanStd), normalize_advantage over the batch
  schedule        linear learning rate from 1e-4 to rl_games' LinearScheduler default minimum 1e-6 over max_epochs
Prints step fps, total fps, the mean disc reward and the discriminator's logged values per epoch.

Checkpoints (isaacgymdyros_amd/amp_checkpoint.py, the reference learner's layout; common_agent.py:65-67, 124, 172-178): with --output_dir,
<output_dir>/<name>/nn/<name>_<epoch>.pth every --save_frequency completed epochs and <name>.pth at the end (<name>: TocabiAMPLower).  With
--checkpoint the run resumes from such a file: weights, normalisers, both Adam states, the AMP buffers and the learning-rate schedule; the
epoch numbering continues and --epochs more epochs run.

--policy_backend hip runs the actor-critic on isaacgymdyros_amd/amp_policy.py's AmpActorCritic instead (the rollout forward, the bootstrap
values, GAE, the value normaliser and the minibatch updates on the dwa_ kernels); the default, torch, is the inline loop below.

--episode-stats switches on the env's on-GPU episode statistics (cfg sim.mi355.amp_episode_stats, isaacgymdyros_amd/amp_episode_stats.py) for
either policy backend: one more line per epoch -- the termination causes, the three most frequent contact bodies, the mean episode length
and return over that epoch's rollout -- and the window restarted per epoch.

--game-meter runs the learner's episode-return meter (isaacgymdyros_amd/game_meter.py; the reference's game_rewards and game_lengths over the
last 100 finished episodes, amp_continuous.py:126-143, common_agent.py:158-168) for either policy backend: one launch after every env.step,
fed the raw task reward (before reward_scale), and `mean_rewards`, `episode length` and `games` at the end of the epoch line.  The window
slides over the run.  There are no best files for this learner (common_agent.py has none); last_mean_rewards goes from a checkpoint into
the files written.
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import tempfile
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from isaacgymdyros_amd import amp_checkpoint as CK    # noqa: E402
from isaacgymdyros_amd import amp_disc as AD          # noqa: E402
from isaacgymdyros_amd import amp_policy as AP        # noqa: E402


def mlp(n_in, units):
    layers = []
    for u in units:
        layers += [nn.Linear(n_in, u), nn.ReLU()]
        n_in = u
    return nn.Sequential(*layers), n_in


class ActorCritic(nn.Module):
    def __init__(self, num_obs, num_act, units, sigma_init):
        super().__init__()
        self.actor_mlp, n = mlp(num_obs, units)
        self.critic_mlp, _ = mlp(num_obs, units)
        self.mu, self.value = nn.Linear(n, num_act), nn.Linear(n, 1)
        self.sigma = nn.Parameter(torch.full((num_act,), float(sigma_init)), requires_grad=False)
        self.obs_rms, self.value_rms = AD.RunningMeanStd(num_obs), AD.RunningMeanStd(1)

    def forward(self, obs):
        x = self.obs_rms(obs)
        return self.mu(self.actor_mlp(x)), self.value(self.critic_mlp(x))

    def neglogp(self, a, mu):
        s = self.sigma
        return 0.5 * (((a - mu) / torch.exp(s)) ** 2).sum(-1) + 0.5 * math.log(2 * math.pi) * a.shape[-1] + s.sum()

    def unnorm_value(self, v):
        r = self.value_rms
        return v * torch.sqrt(r.running_var.float() + r.epsilon) + r.running_mean.float()


def make_env(n, device, motion_file, synthetic, motion_device=False, episode_stats=False):
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    cfg = default_amp_cfg(n, device)
    if synthetic:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import amp_motion_synth as SY
        motion_file = SY.write(tempfile.mkdtemp(prefix="amp_synth_"))
    if not motion_file:
        raise SystemExit("give --motion_file (the task's motion yaml) or --synthetic")
    cfg["env"]["motion_file"] = motion_file
    if motion_device:          # the motion library as a table on the device: fetch_amp_obs_demo is one launch (sim.mi355.amp_motion_device)
        cfg["sim"].setdefault("mi355", {})["amp_motion_device"] = True
    if episode_stats:
        cfg["sim"].setdefault("mi355", {})["amp_episode_stats"] = True
    return TocabiAMPLower(cfg, device, 0, True)


def episode_line(env, epoch):
    """--episode-stats: the epoch's window as one line; the next epoch starts a new one."""
    if env.episode_stats is None:
        return
    from isaacgymdyros_amd.amp_episode_stats import format_line
    print("epoch %d: %s" % (epoch, format_line(env.episode_stats.summary())), flush=True)
    env.episode_stats.reset_totals()


def make_meter(args, N, dev):
    """--game-meter: the learner's GameMeter, or None."""
    if not getattr(args, "game_meter", False):
        return None
    from isaacgymdyros_amd.game_meter import GameMeter
    return GameMeter(N, dev, cols=1, games_to_track=100)


def meter_text(meter):
    """The end of the epoch line: empty without --game-meter."""
    if meter is None:
        return ""
    m = meter.summary()          # (one device-to-host copy; the epoch's synchronisation is behind us)
    if not (math.isfinite(m["mean_reward"]) and math.isfinite(m["mean_length"])):
        raise SystemExit("non-finite episode return or length in the game meter")
    return "  mean_rewards %.4f  episode length %.1f  games %d" % (m["mean_reward"], m["mean_length"], m["games"])


class Checkpoints:
    """--checkpoint / --output_dir / --save_frequency for one run: resume() before the first epoch, after_epoch() after each, finish() at the end."""

    def __init__(self, args, N, H, lr0, lr_min, max_epochs):
        self.args, self.rows = args, N * H
        self.sched = {"lr0": lr0, "lr_min": lr_min, "max_epochs": max_epochs}
        self.dir = os.path.join(args.output_dir, CK.NAME, "nn") if args.output_dir else None
        self.freq = args.save_frequency
        # --game-meter: a checkpoint's last_mean_rewards goes into the files written (this learner never moves it: common_agent.py)
        self.last_mean_rewards = CK.LAST_MEAN_REWARDS if getattr(args, "game_meter", False) else None
        if self.freq is None:
            self.freq = CK.SAVE_FREQUENCY
            if args.train_yaml:
                import yaml
                self.freq = int(yaml.safe_load(open(args.train_yaml))["params"]["config"].get("save_frequency", CK.SAVE_FREQUENCY))

    def resume(self, policy, disc) -> int:
        """The first epoch of this run (0, or the checkpoint's completed epochs); the schedule continues with the checkpoint's values."""
        if not self.args.checkpoint:
            return 0
        c = CK.restore(self.args.checkpoint, policy, disc)
        for k in self.sched:
            if c[k] is not None:
                self.sched[k] = c[k]
        if self.last_mean_rewards is not None:
            self.last_mean_rewards = c["last_mean_rewards"]
        print("resumed %s at epoch %d" % (self.args.checkpoint, c["epoch"]), flush=True)
        return c["epoch"]

    def lr(self, epoch):
        s = self.sched
        return s["lr_min"] + (s["lr0"] - s["lr_min"]) * max(0, s["max_epochs"] - epoch) / s["max_epochs"]

    def _save(self, name, policy, disc, done):
        more = {} if self.last_mean_rewards is None else {"last_mean_rewards": self.last_mean_rewards}
        path = CK.save(os.path.join(self.dir, name + ".pth"), policy, disc, done, done * self.rows, **self.sched, **more)
        print("saved %s epoch %d lr %.9e" % (path, done, policy.optimizer_state()["lr"]), flush=True)

    def after_epoch(self, epoch, policy, disc):
        done = epoch + 1
        if self.dir and self.freq > 0 and done % self.freq == 0:
            self._save("%s_%d" % (CK.NAME, done), policy, disc, done)

    def finish(self, epoch_end, policy, disc):
        if self.dir:
            self._save(CK.NAME, policy, disc, epoch_end)


def train(args):
    tc = AD.load_train_yaml(args.train_yaml) if args.train_yaml else AD.TRAIN_CFG
    c, netc = tc["config"], tc["network"]
    dev = torch.device(args.device)
    env = make_env(args.num_envs, args.device, args.motion_file, args.synthetic, args.motion_device, getattr(args, "episode_stats", False))
    N, H, A = env.num_envs, int(c["horizon_length"]), env.num_actions
    lr0, lr_min, max_epochs = float(c["learning_rate"]), 1e-6, int(args.max_epochs or c["max_epochs"])
    if args.policy_backend == "hip":
        return train_hip(args, tc, dev, env, N, H, A, lr0, lr_min, max_epochs)
    model = ActorCritic(env.num_obs, A, netc["mlp_units"], netc["sigma_init"]).to(dev)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=lr0, eps=1e-8)
    disc = AD.AmpDiscriminator(env.num_amp_obs, dev, tc, backend=args.backend)
    disc.init_demo_buffer(env.fetch_amp_obs_demo)
    gamma, tau, e_clip = float(c["gamma"]), float(c["tau"]), float(c["e_clip"])
    mb = {"obs": torch.zeros(H, N, env.num_obs, device=dev), "act": torch.zeros(H, N, A, device=dev), "mu": torch.zeros(H, N, A, device=dev),
          "nlp": torch.zeros(H, N, device=dev), "val": torch.zeros(H, N, 1, device=dev), "next_val": torch.zeros(H, N, 1, device=dev),
          "rew": torch.zeros(H, N, 1, device=dev), "done": torch.zeros(H, N, device=dev), "amp": torch.zeros(H, N, env.num_amp_obs, device=dev)}
    ckp, learner = Checkpoints(args, N, H, lr0, lr_min, max_epochs), CK.TorchLearner(model, opt)
    first = ckp.resume(learner, disc)
    meter = make_meter(args, N, dev)
    env.reset()
    for epoch in range(first, first + args.epochs):
        lr = ckp.lr(epoch)
        for g in opt.param_groups:
            g["lr"] = lr
        t0 = time.time()
        step_time = 0.0
        model.eval()
        with torch.no_grad():                                        # play_steps
            for n in range(H):
                obs = env.reset_done()[0]["obs"]
                mu, v = model(obs)
                act = mu + torch.exp(model.sigma) * torch.randn_like(mu)
                mb["obs"][n], mb["act"][n], mb["mu"][n], mb["nlp"][n], mb["val"][n] = obs, act, mu, model.neglogp(act, mu), model.unnorm_value(v)
                ts = time.time()
                obs2, rew, done, infos = env.step(torch.clamp(act, -1.0, 1.0))
                torch.cuda.synchronize(dev)
                step_time += time.time() - ts
                if meter is not None:
                    meter.record(rew, done)
                mb["rew"][n], mb["done"][n], mb["amp"][n] = rew.view(N, 1) * float(c["reward_scale"]), done.float(), infos["amp_obs"]
                nv = model.unnorm_value(model(obs2["obs"])[1])
                mb["next_val"][n] = nv * (1.0 - infos["terminate"].float().view(N, 1))
            combined, disc_r = disc.rewards(mb["amp"], mb["rew"])     # _calc_amp_rewards + _combine_rewards
            adv = torch.zeros_like(combined)
            last = torch.zeros(N, 1, device=dev)
            for t in reversed(range(H)):
                delta = combined[t] + gamma * mb["next_val"][t] - mb["val"][t]
                last = delta + gamma * tau * (1.0 - mb["done"][t]).view(N, 1) * last
                adv[t] = last
            ret = adv + mb["val"]
        flat = lambda x: x.transpose(0, 1).reshape(N * H, *x.shape[2:])          # noqa: E731 (swap_and_flatten01)
        obs_b, act_b, nlp_b, val_b, amp_b = (flat(mb[k]) for k in ("obs", "act", "nlp", "val", "amp"))
        ret_b = flat(ret)
        disc.update_demos(env.fetch_amp_obs_demo)
        demo_b = disc.demo_buffer.sample(N * H)
        replay_b = disc.replay_batch(amp_b)
        with torch.no_grad():                                        # prepare_dataset: value normalisation, advantage normalisation
            model.value_rms.train()
            val_n, ret_n = model.value_rms(val_b), model.value_rms(ret_b)
            model.value_rms.eval()
            adv_b = ret_b - val_b
            adv_b = (adv_b - adv_b.mean()) / (adv_b.std() + 1e-8)
        model.train()
        model.value_rms.eval()
        B = min(int(c["minibatch_size"]), N * H)
        amb = min(int(c["amp_minibatch_size"]), B)
        losses = []
        for _ in range(int(c["mini_epochs"])):
            for i in range(0, N * H - B + 1, B):
                s = slice(i, i + B)
                mu, v = model(obs_b[s])
                ratio = torch.exp(nlp_b[s] - model.neglogp(act_b[s], mu))
                a = adv_b[s].view(-1)
                a_loss = torch.max(-a * ratio, -a * torch.clamp(ratio, 1 - e_clip, 1 + e_clip)).mean()
                c_loss = ((ret_n[s] - v) ** 2).mean()
                b_loss = ((torch.clamp(mu - 1.0, min=0) ** 2 + torch.clamp(mu + 1.0, max=0) ** 2).sum(-1)).mean()
                loss = a_loss + float(c["critic_coef"]) * c_loss + float(c["bounds_loss_coef"]) * b_loss
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
                disc.update(amp_b[s][:amb].contiguous(), replay_b[s][:amb].contiguous(), demo_b[s][:amb].contiguous(), lr=lr)
                losses.append(torch.stack([a_loss.detach(), c_loss.detach(), b_loss.detach()]))
        disc.store_replay(amp_b)
        torch.cuda.synchronize(dev)
        total = time.time() - t0
        info = disc.pop_info()
        al, cl, bl = torch.stack(losses).mean(0).tolist()
        print("epoch %d  step fps %.0f  total fps %.0f  disc_r %.4f  a_loss %.4f  c_loss %.4f  b_loss %.4f  %s%s"
              % (epoch, N * H / max(step_time, 1e-9), N * H / total, float(disc_r.mean()), al, cl, bl,
                 "  ".join("%s %.4f" % (k.replace("disc_", ""), v) for k, v in info.items()), meter_text(meter)), flush=True)
        episode_line(env, epoch)
        vals = [al, cl, bl, float(disc_r.mean()), float(combined.mean())] + list(info.values())
        if not all(math.isfinite(x) for x in vals):
            raise SystemExit("non-finite loss or reward at epoch %d" % epoch)
        ckp.after_epoch(epoch, learner, disc)
    ckp.finish(first + args.epochs, learner, disc)


def train_hip(args, tc, dev, env, N, H, A, lr0, lr_min, max_epochs):
    """train() with the actor-critic on AmpActorCritic's kernels; the same epoch structure and the same printed line."""
    c = tc["config"]
    pol = AP.AmpActorCritic(env.num_obs, A, dev, tc, backend="hip")
    disc = AD.AmpDiscriminator(env.num_amp_obs, dev, tc, backend=args.backend)
    disc.init_demo_buffer(env.fetch_amp_obs_demo)
    gamma, tau = float(c["gamma"]), float(c["tau"])
    mb = {"obs": torch.zeros(H, N, env.num_obs, device=dev), "act": torch.zeros(H, N, A, device=dev), "nlp": torch.zeros(H, N, device=dev),
          "val": torch.zeros(H, N, 1, device=dev), "next_val": torch.zeros(H, N, 1, device=dev), "rew": torch.zeros(H, N, 1, device=dev),
          "done": torch.zeros(H, N, device=dev), "amp": torch.zeros(H, N, env.num_amp_obs, device=dev)}
    ckp = Checkpoints(args, N, H, lr0, lr_min, max_epochs)
    first = ckp.resume(pol, disc)
    meter = make_meter(args, N, dev)
    env.reset()
    for epoch in range(first, first + args.epochs):
        lr = ckp.lr(epoch)
        t0 = time.time()
        step_time = 0.0
        with torch.no_grad():                                        # play_steps
            for n in range(H):
                obs = env.reset_done()[0]["obs"].contiguous()
                act, act_c, _mu, nlp, val = pol.act(obs, torch.randn(N, A, device=dev))
                mb["obs"][n], mb["act"][n], mb["nlp"][n], mb["val"][n] = obs, act, nlp, val
                ts = time.time()
                obs2, rew, done, infos = env.step(act_c)
                torch.cuda.synchronize(dev)
                step_time += time.time() - ts
                if meter is not None:
                    meter.record(rew, done)
                mb["rew"][n], mb["done"][n], mb["amp"][n] = rew.view(N, 1) * float(c["reward_scale"]), done.float(), infos["amp_obs"]
                mb["next_val"][n] = pol.eval_critic(obs2["obs"].contiguous(), infos["terminate"].float().contiguous())
            combined, disc_r = disc.rewards(mb["amp"], mb["rew"])     # _calc_amp_rewards + _combine_rewards
            _adv, ret = AP.gae(mb["done"], mb["val"], combined, mb["next_val"], gamma, tau)
        flat = lambda x: x.transpose(0, 1).reshape(N * H, *x.shape[2:])          # noqa: E731 (swap_and_flatten01)
        obs_b, act_b, nlp_b, val_b, amp_b = (flat(mb[k]) for k in ("obs", "act", "nlp", "val", "amp"))
        ret_b = flat(ret)
        disc.update_demos(env.fetch_amp_obs_demo)
        demo_b = disc.demo_buffer.sample(N * H)
        replay_b = disc.replay_batch(amp_b)
        with torch.no_grad():                                        # prepare_dataset: value normalisation, advantage normalisation
            ret_n = pol.update_value_stats(val_b, ret_b).reshape(-1)
            adv_b = ret_b - val_b
            adv_b = ((adv_b - adv_b.mean()) / (adv_b.std() + 1e-8)).reshape(-1)
        B = min(int(c["minibatch_size"]), N * H)
        amb = min(int(c["amp_minibatch_size"]), B)
        for _ in range(int(c["mini_epochs"])):
            for i in range(0, N * H - B + 1, B):
                s = slice(i, i + B)
                pol.update(obs_b[s], act_b[s], nlp_b[s], adv_b[s], ret_n[s], lr=lr)
                disc.update(amp_b[s][:amb].contiguous(), replay_b[s][:amb].contiguous(), demo_b[s][:amb].contiguous(), lr=lr)
        disc.store_replay(amp_b)
        torch.cuda.synchronize(dev)
        total = time.time() - t0
        info, pinfo = disc.pop_info(), pol.pop_info()
        al, cl, bl = pinfo["a_loss"], pinfo["c_loss"], pinfo["b_loss"]
        print("epoch %d  step fps %.0f  total fps %.0f  disc_r %.4f  a_loss %.4f  c_loss %.4f  b_loss %.4f  %s%s"
              % (epoch, N * H / max(step_time, 1e-9), N * H / total, float(disc_r.mean()), al, cl, bl,
                 "  ".join("%s %.4f" % (k.replace("disc_", ""), v) for k, v in info.items()), meter_text(meter)), flush=True)
        episode_line(env, epoch)
        vals = [al, cl, bl, float(disc_r.mean()), float(combined.mean())] + list(info.values())
        if not all(math.isfinite(x) for x in vals):
            raise SystemExit("non-finite loss or reward at epoch %d" % epoch)
        ckp.after_epoch(epoch, pol, disc)
    ckp.finish(first + args.epochs, pol, disc)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--max_epochs", type=int, default=0, help="of the learning-rate schedule (default: the yaml's)")
    ap.add_argument("--motion_file", default=None)
    ap.add_argument("--synthetic", action="store_true", help="the synthetic motion tables of tests/amp_motion_synth.py")
    ap.add_argument("--motion-device", dest="motion_device", action="store_true",
                    help="sim.mi355.amp_motion_device: the motion library on the device (demonstration fetches and reference starts without the host)")
    ap.add_argument("--train_yaml", default=None, help="cfg/train/TocabiAMPLowerPPO.yaml (default: the built-in copy of its values)")
    ap.add_argument("--backend", default="hip", choices=["hip", "torch"])
    ap.add_argument("--policy_backend", default="torch", choices=["torch", "hip"], help="the actor-critic: the inline torch loop or AmpActorCritic")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--output_dir", default=None, help="write checkpoints under <output_dir>/TocabiAMPLower/nn (default: none are written)")
    ap.add_argument("--save_frequency", type=int, default=None, help="a checkpoint every this many epochs (default: the yaml's, 100)")
    ap.add_argument("--checkpoint", default=None, help="resume from this checkpoint")
    ap.add_argument("--episode-stats", dest="episode_stats", action="store_true",
                    help="sim.mi355.amp_episode_stats: one more line per epoch with the termination causes, contact bodies, episode length and return")
    ap.add_argument("--game-meter", dest="game_meter", action="store_true",
                    help="the learner's on-GPU episode-return meter: mean_rewards, episode length and games at the end of the epoch line")
    train(ap.parse_args())


if __name__ == "__main__":
    main()
