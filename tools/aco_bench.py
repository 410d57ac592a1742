"""End-to-end time of the Ant System search (rl4co_amd.aco.AntSystem on csrc/aco_tsp.hip) at DeepACO's defaults: 4096 x
TSP-100, 48 ants, 10 iterations, heuristic -log(distance). Three legs, alternating round by round after one warm-up round,
each timed with HIP events around the whole ``run`` (host work included) and synchronised:
  fused          one rl4co_aco_tsp launch for all iterations
  local_search   per iteration: SAMPLE launch, the 2-opt kernel, the reward kernel, UPDATE launch
  torch_per_step the same configuration composed per decoding step from torch ops on the GPU — this script's own plain
                 restatement of the loop (one multinomial draw per step, a Python loop over the ants in the deposit), for
                 scale only: it draws other tours than the kernel.
Next to the times: the mean best tour length after the last iteration, in float64.

    python tools/aco_bench.py [--reps 5] [--batch 4096] [--num-loc 100] [--out profiles/aco_bench.json]

``--env cvrp`` times the CVRP search (csrc/aco_cvrp.hip) instead: 4096 x CVRP-100 from the environment's generator, 48 ants,
10 iterations, ``multisample`` decoding (every ant starts at the depot), heuristic -log(distance). One leg, ``fused``: there
is no earlier CVRP path to compare with. Writes profiles/aco_cvrp_bench.json unless ``--out`` says otherwise.

``--env prize`` times the OP and PCTSP search (csrc/aco_prize.hip): 256 x OP-50 and 256 x PCTSP-50 from the environments'
generators (``--batch`` / ``--num-loc`` when given), 48 ants, 10 iterations, ``multisample`` decoding, heuristic
-log(distance). Two legs per environment, alternating: ``fused`` (one rl4co_aco_prize launch) and ``torch_per_step`` (this
script's torch loop over the decoding steps with the environment's mask, for scale only). Next to the times: the mean best
reward after the last iteration. Writes profiles/aco_prize_bench.json unless ``--out`` says otherwise.

``--nls`` times one iteration's neural-guided local search (csrc/tsp_nls.hip) instead: 1024 x TSP-100, 20 ants, 5
perturbations of at most 5 scans; the fused launch against the composition of the 2-opt and reward kernels on the same
tours (``main_nls``). Writes profiles/aco_nls_bench.json unless ``--out`` says otherwise.

``--train`` times DeepACO's training decode instead (csrc/aco_tsp.hip SAMPLE + csrc/aco_tsp_grad.hip): forward plus
backward of the ants' log-likelihoods from a free heatmap at TSP-100 x 30 ants, for a batch below (64) and a batch above
(512) the card's CU count; ``kernels`` (``heatmap_rollout``: two launches) against ``torch_per_step`` (the step loop in
torch ops with autograd on the same card, what the reference executes), alternating (``main_train``). No threshold: both
times and their ratio are reported. Writes profiles/aco_train_bench.json unless ``--out`` says otherwise.
``--train --env cvrp|op|pctsp`` is the same protocol on a depot graph (csrc/aco_cvrp.hip / csrc/aco_prize.hip SAMPLE +
csrc/aco_depot_grad.hip) with 100 customers, every ant starting at the depot (``main_train_depot``); all three rows are
merged into profiles/aco_depot_train_bench.json unless ``--out`` says otherwise.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rl4co_amd import AntSystem  # noqa: E402
from rl4co_amd.envs import get_env  # noqa: E402
from rl4co_amd.tensordict import TensorDict  # noqa: E402


def length64(locs, tours):
    p = locs.double().gather(1, tours[..., None].expand(-1, -1, 2))
    return (p - p.roll(-1, dims=1)).norm(dim=-1).sum(1)


def torch_ant_system(heu, locs, n_ants, iterations, alpha=1.0, beta=1.0, decay=0.95):
    """The Ant System loop from torch ops, one decoding step at a time (ant-major rows)."""
    b, n, _ = heu.shape
    rows = n_ants * b
    q = 1 / n_ants / decay
    dev = heu.device
    ar, inst = torch.arange(rows, device=dev), torch.arange(rows, device=dev) % b
    bidx = torch.arange(b, device=dev)
    phe = torch.ones_like(heu)
    best_reward = best_actions = None
    for _ in range(iterations):
        logits = alpha * torch.log(phe) + beta * heu
        cur = (ar // b) % n
        mask = torch.ones(rows, n, dtype=torch.bool, device=dev)
        mask[ar, cur] = False
        steps = [cur]
        for _t in range(1, n):
            lp = torch.log_softmax(logits[inst, cur].masked_fill(~mask, float("-inf")), -1)
            cur = torch.multinomial(lp.exp(), 1).squeeze(1)
            mask[ar, cur] = False
            steps.append(cur)
        actions = torch.stack(steps, 1)
        pts = locs[inst[:, None], actions]
        reward = -(pts.roll(-1, 1) - pts).norm(p=2, dim=-1).sum(1)
        rew, act = reward.view(n_ants, b).t(), actions.view(n_ants, b, n)
        top = rew.argmax(-1)
        top_reward, top_actions = rew[bidx, top], act[top, bidx]
        if best_reward is None:
            best_reward, best_actions = top_reward.clone(), top_actions.clone()
        else:
            take = best_reward <= top_reward
            best_reward = torch.where(take, top_reward, best_reward)
            best_actions = torch.where(take[:, None], top_actions, best_actions)
        hi, lo = rew.max(-1, keepdim=True).values, rew.min(-1, keepdim=True).values
        v = ((rew - lo) / (hi - lo)) ** 2 * q
        delta = torch.zeros_like(phe)
        for j in range(n_ants):
            delta[bidx[:, None], act[j, :, :-1], act[j, :, 1:]] += v[:, j : j + 1]
        delta[:, 0, 0] = 0
        phe = phe * decay + delta
    return best_actions


def cvrp_length64(locs, tours):
    """Closed length of [depot, tours] in float64 (trailing depot visits add nothing)."""
    return length64(locs, torch.cat((torch.zeros_like(tours[:, :1]), tours), 1))


class Leg:
    def __init__(self, kind, fn, length=length64):
        self.kind, self.fn, self.times, self.tours, self.length = kind, fn, [], None, length

    def launch(self, keep: bool):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.tours = self.fn()
        e1.record()
        torch.cuda.synchronize()
        if keep:
            self.times.append(e0.elapsed_time(e1))

    def result(self, locs):
        t = sorted(self.times)
        return dict(leg=self.kind, reps=len(t), median_ms=t[len(t) // 2], min_ms=t[0], max_ms=t[-1],
                    mean_best_length_f64=float(self.length(locs, self.tours).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="default 4096 (--train: 64 and 512)")
    ap.add_argument("--num-loc", type=int, default=100)
    ap.add_argument("--ants", type=int, default=None, help="default 48 (--train: 30)")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--env", choices=("tsp", "cvrp", "prize", "op", "pctsp"), default="tsp", help="op / pctsp: with --train")
    ap.add_argument("--nls", action="store_true", help="time the neural-guided local search instead (TSP)")
    ap.add_argument("--train", action="store_true", help="time the training decode, forward plus backward, instead (TSP)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aco_bench needs the MI355X: a time taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    if a.train:  # its own defaults: an explicit --ants / --batch is taken as given
        return main_train(a, dev) if a.env == "tsp" else main_train_depot(a, dev)
    if a.env in ("op", "pctsp"):
        raise SystemExit("aco_bench --env op / pctsp goes with --train (the search of both is --env prize)")
    a.batch = 4096 if a.batch is None else a.batch
    a.ants = 48 if a.ants is None else a.ants
    if a.env == "cvrp":
        return main_cvrp(a, dev)
    if a.env == "prize":
        return main_prize(a, dev)
    if a.nls:
        return main_nls(a, dev)
    g = torch.Generator().manual_seed(1234)
    locs = torch.rand(a.batch, a.num_loc, 2, generator=g).to(dev)
    dist = (locs[:, :, None] - locs[:, None, :]).norm(p=2, dim=-1)
    heu = -torch.log(dist + 1e9 * torch.eye(a.num_loc, device=dev))
    env = get_env("tsp", generator_params=dict(num_loc=a.num_loc, device=dev), device=dev)
    td = env.reset(TensorDict({"locs": locs}, batch_size=[a.batch]))
    kwargs = dict(multistart=True, num_starts=a.ants, select_best=False)

    def kernel_run(**kw):
        def run():
            torch.manual_seed(0)
            return AntSystem(heu, n_ants=a.ants, **kw).run(td, env, a.iterations, kwargs)[0]

        return run

    legs = [Leg("fused", kernel_run()), Leg("local_search", kernel_run(use_local_search=True)),
            Leg("torch_per_step", lambda: torch_ant_system(heu, locs, a.ants, a.iterations))]
    for it in range(a.reps + 1):  # one warm-up round; the legs alternate inside every round
        for leg in legs:
            leg.launch(keep=it >= 1)
    rows = [leg.result(locs) for leg in legs]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), when=time.strftime("%Y-%m-%d"),
                           case=f"tsp{a.num_loc}x{a.batch}, {a.ants} ants, {a.iterations} iterations",
                           what="AntSystem.run end to end (host work included), HIP events around the call, synchronised",
                           rows=rows), f, indent=1)


def main_cvrp(a, dev):
    torch.manual_seed(1234)
    env = get_env("cvrp", generator_params=dict(num_loc=a.num_loc, device=dev), device=dev)
    td = env.reset(batch_size=[a.batch])
    locs = td["locs"]  # [B, num_loc + 1, 2], the depot first
    dist = (locs[:, :, None] - locs[:, None, :]).norm(p=2, dim=-1)
    heu = -torch.log(dist + 1e9 * torch.eye(a.num_loc + 1, device=dev))
    kwargs = dict(multisample=True, num_samples=a.ants, select_best=False)

    def run():
        torch.manual_seed(0)
        return AntSystem(heu, n_ants=a.ants).run(td, env, a.iterations, kwargs)[0]

    leg = Leg("fused", run, cvrp_length64)
    for it in range(a.reps + 1):  # one warm-up round
        leg.launch(keep=it >= 1)
    env.check_solution_validity(td, leg.tours)
    row = leg.result(locs)
    print(json.dumps(row), flush=True)
    out = a.out or "profiles/aco_cvrp_bench.json"
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), when=time.strftime("%Y-%m-%d"),
                       case=f"cvrp{a.num_loc}x{a.batch}, {a.ants} ants, {a.iterations} iterations, multisample",
                       what="AntSystem.run end to end (host work included), HIP events around the call, synchronised",
                       rows=[row]), f, indent=1)


def torch_prize_ant_system(name, heu, td, n_ants, iterations, alpha=1.0, beta=1.0, decay=0.95):
    """The Ant System loop for OP / PCTSP from torch ops, one decoding step at a time (ant-major rows, the environment's mask
    and reward in its own expressions). Returns the best reward per instance."""
    b, n, _ = heu.shape
    rows, q, dev = n_ants * b, 1 / n_ants / decay, heu.device
    ar, inst = torch.arange(rows, device=dev), torch.arange(rows, device=dev) % b
    bidx = torch.arange(b, device=dev)
    locs = td["locs"][inst]
    prize = td["prize" if name == "op" else "real_prize"][inst]
    limit = td["max_length"][inst] if name == "op" else None
    penalty = td["penalty"][inst] if name != "op" else None
    phe = torch.ones_like(heu)
    best_reward = None
    for _ in range(iterations):
        logits = alpha * torch.log(phe) + beta * heu
        cur = torch.zeros(rows, dtype=torch.int64, device=dev)
        visited = torch.zeros(rows, n, dtype=torch.bool, device=dev)
        acc = torch.zeros(rows, device=dev)
        done = torch.zeros(rows, dtype=torch.bool, device=dev)
        steps = []
        for t in range(n):
            mask = visited | visited[:, 0:1]
            if name == "op":
                mask = mask | (acc[:, None] + (locs - locs[ar, cur][:, None, :]).norm(p=2, dim=-1) > limit)
                mask[:, 0] = False
            else:
                mask[:, 0] = (acc < 1.0) & (visited[:, 1:].sum(-1) < n - 1)
            lp = torch.log_softmax(logits[inst, cur].masked_fill(mask, float("-inf")), -1)
            nxt = torch.where(done, torch.zeros_like(cur), torch.multinomial(lp.exp(), 1).squeeze(1))
            acc = acc + ((locs[ar, nxt] - locs[ar, cur]).norm(p=2, dim=-1) if name == "op" else prize[ar, nxt])
            visited[ar, nxt] = True
            done = done | ((nxt == 0) & (t > 0))
            cur = nxt
            steps.append(nxt)
        actions = torch.stack(steps, 1)
        if name == "op":
            reward = prize.gather(1, actions).sum(-1)
        else:
            pts = locs[ar[:, None], torch.cat((torch.zeros_like(actions[:, :1]), actions), 1)]
            length = (pts.roll(-1, 1) - pts).norm(p=2, dim=-1).sum(1)
            reward = penalty.gather(1, actions).sum(-1) - (length + penalty[:, 1:].sum(-1))
        rew, act = reward.view(n_ants, b).t(), actions.view(n_ants, b, n)
        top_reward = rew.max(-1).values
        best_reward = top_reward.clone() if best_reward is None else torch.maximum(best_reward, top_reward)
        hi, lo = rew.max(-1, keepdim=True).values, rew.min(-1, keepdim=True).values
        v = ((rew - lo) / (hi - lo)) ** 2 * q
        delta = torch.zeros_like(phe)
        for j in range(n_ants):
            delta[bidx[:, None], act[j, :, :-1], act[j, :, 1:]] += v[:, j : j + 1]
        delta[:, 0, 0] = 0
        phe = phe * decay + delta
    return best_reward


def main_prize(a, dev):
    batch = a.batch if a.batch != 4096 else 256  # (the defaults of this script are sized for TSP-100)
    num_loc = a.num_loc if a.num_loc != 100 else 50
    kwargs = dict(multisample=True, num_samples=a.ants, select_best=False)
    rows = []
    for name in ("op", "pctsp"):
        torch.manual_seed(1234)
        env = get_env(name, generator_params=dict(num_loc=num_loc, device=dev), device=dev)
        td = env.reset(batch_size=[batch])
        locs = td["locs"]  # [B, num_loc + 1, 2], the depot first
        dist = (locs[:, :, None] - locs[:, None, :]).norm(p=2, dim=-1)
        heu = -torch.log(dist + 1e9 * torch.eye(num_loc + 1, device=dev))
        state = {}

        def fused():
            torch.manual_seed(0)
            aco = AntSystem(heu, n_ants=a.ants)
            state["tours"] = aco.run(td, env, a.iterations, kwargs)[0]
            return aco.final_reward

        def per_step():
            torch.manual_seed(0)
            return torch_prize_ant_system(name, heu, td, a.ants, a.iterations)

        legs = [Leg("fused", fused, lambda _locs, reward: reward.double()),
                Leg("torch_per_step", per_step, lambda _locs, reward: reward.double())]
        for it in range(a.reps + 1):  # one warm-up round; the legs alternate inside every round
            for leg in legs:
                leg.launch(keep=it >= 1)
        env.check_solution_validity(td, state["tours"])
        for leg in legs:
            row = leg.result(locs)
            row = dict(env=name, case=f"{name}{num_loc}x{batch}", **row)
            row["mean_best_reward_f64"] = row.pop("mean_best_length_f64")
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = a.out or "profiles/aco_prize_bench.json"
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), when=time.strftime("%Y-%m-%d"),
                       case=f"op{num_loc} and pctsp{num_loc} x {batch}, {a.ants} ants, {a.iterations} iterations, multisample",
                       what="AntSystem.run end to end (host work included), HIP events around the call, synchronised; "
                            "torch_per_step is this script's torch loop on the same card, for scale only",
                       rows=rows), f, indent=1)


def main_nls(a, dev):
    """``--nls``: the neural-guided local search of ONE iteration at DeepACO's own shape (TSP-100, 20 ants, 5 perturbations
    of at most 5 scans), on the tours a SAMPLE launch drew. Two legs on the same inputs, alternating round by round after one
    warm-up round, min and median of ``--reps`` repeats, HIP events around the call (host work included), synchronised:
      fused        AntSystem(use_nls=True).local_search: one rl4co_tsp_nls launch
      composition  the same search written with the kernels merged before it: 1 + 2 P rl4co_tsp_two_opt launches over
                   matrices tiled per ant, as many reward launches, compare / select glue in torch
    The two must agree bit for bit (checked here before anything is written)."""
    from rl4co_amd import _lib
    from rl4co_amd import kernels as K

    batch = a.batch if a.batch != 4096 else 1024  # (the TSP default of this script is sized for the sampling kernel)
    ants, n, n_pert, pert_cap = 20, a.num_loc, 5, 5
    g = torch.Generator().manual_seed(1234)
    locs = torch.rand(batch, n, 2, generator=g).to(dev)
    dist = (locs[:, :, None] - locs[:, None, :]).norm(p=2, dim=-1)
    heu = -torch.log(dist + 1e9 * torch.eye(n, device=dev))
    env = get_env("tsp", generator_params=dict(num_loc=n, device=dev), device=dev)
    td = env.reset(TensorDict({"locs": locs}, batch_size=[batch]))
    aco = AntSystem(heu, n_ants=ants, use_local_search=True, use_nls=True, n_perturbations=n_pert,
                    perturbation_params={"max_iterations": pert_cap})
    starts = aco._start_nodes(td, env, {})[None].contiguous()
    sampled = K.aco_tsp(aco.pheromone, n_ants=ants, phases=_lib.ACO_SAMPLE, log_heuristic=heu, locs=locs, start_nodes=starts,
                        philox_seed=1234)["actions"]
    pert = aco.heuristic_dist
    rows = sampled.shape[0]

    def fused():
        return aco.local_search(td, env, sampled, {})

    def composition():  # one error word and one read-back, as the fused leg has; no validity check, as the fused leg has none
        err = K.new_error_word(dev)
        tiled = {"locs": locs.repeat(rows // batch, 1, 1)}
        tiled_pert = pert.repeat(rows // batch, 1, 1)
        cur = K.tsp_two_opt(sampled, locs=tiled["locs"], err=err)
        best, best_r = cur.clone(), env.get_reward(tiled, cur, check_solution=False)
        for _ in range(n_pert):
            cur = K.tsp_two_opt(cur, distances=tiled_pert, max_iterations=pert_cap, err=err)
            cur = K.tsp_two_opt(cur, locs=tiled["locs"], err=err)
            r = env.get_reward(tiled, cur, check_solution=False)
            win = r > best_r
            best, best_r = torch.where(win[:, None], cur, best), torch.where(win, r, best_r)
        K.raise_if_error(err)
        return best, best_r

    legs = [Leg("fused", fused), Leg("composition", composition)]
    for it in range(a.reps + 1):  # one warm-up round; the legs alternate inside every round
        for leg in legs:
            leg.launch(keep=it >= 1)
    (fa, fr), (ca, cr) = legs[0].tours, legs[1].tours
    if not (torch.equal(fa, ca) and torch.equal(fr, cr)):
        raise SystemExit("aco_bench --nls: the fused launch and the composition disagree; no time is recorded")
    out_rows = []
    for leg in legs:
        t = sorted(leg.times)
        out_rows.append(dict(leg=leg.kind, reps=len(t), median_ms=t[len(t) // 2], min_ms=t[0], max_ms=t[-1],
                             mean_length_f64=float(-leg.tours[1].double().mean())))
        print(json.dumps(out_rows[-1]), flush=True)
    out = a.out or "profiles/aco_nls_bench.json"
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), when=time.strftime("%Y-%m-%d"),
                       case=f"tsp{n}x{batch}, {ants} ants ({rows} tour rows), {n_pert} perturbations of <= {pert_cap} scans, "
                            f"tours from one SAMPLE launch",
                       what="one iteration's neural-guided local search (host work included), HIP events around the call, "
                            "synchronised; the two legs agree bit for bit",
                       rows=out_rows), f, indent=1)


def torch_train_step(heat, locs, n_ants, temperature=1.0):
    """The reference's training decode from torch ops with autograd, one decoding step at a time (ant-major rows): gather
    the row, mask, log-softmax, multinomial, gather the log-prob. Returns (log_likelihood [rows], reward [rows])."""
    b, n, _ = heat.shape
    rows, dev = n_ants * b, heat.device
    ar, inst = torch.arange(rows, device=dev), torch.arange(rows, device=dev) % b
    cur = (ar // b) % n
    mask = torch.ones(rows, n, dtype=torch.bool, device=dev)
    mask[ar, cur] = False
    steps, logps = [cur], []
    for _t in range(1, n):
        lp = torch.log_softmax(heat[inst, cur].masked_fill(~mask, float("-inf")) / temperature, -1)
        cur = torch.multinomial(lp.detach().exp(), 1).squeeze(1)
        logps.append(lp[ar, cur])
        mask = mask.clone()
        mask[ar, cur] = False
        steps.append(cur)
    actions = torch.stack(steps, 1)
    pts = locs[inst[:, None], actions]
    return torch.stack(logps, 1).sum(1), -(pts.roll(-1, 1) - pts).norm(p=2, dim=-1).sum(1)


def main_train(a, dev):
    """``--train``: forward plus backward of DeepACO's training decode from a free heatmap, per batch size two legs
    alternating round by round after one warm-up round, HIP events around forward, loss and backward (host work included),
    synchronised."""
    from rl4co_amd.aco import deepaco_loss, heatmap_rollout

    n = a.num_loc
    ants = 30 if a.ants is None else a.ants  # DeepACO trains with 30 ants
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    batches = (64, 512) if a.batch is None else (a.batch,)
    rows_out = []
    for batch in batches:
        g = torch.Generator().manual_seed(1234)
        locs = torch.rand(batch, n, 2, generator=g).to(dev)
        dist = (locs[:, :, None] - locs[:, None, :]).norm(p=2, dim=-1)
        heat = (-torch.log(dist + 1e9 * torch.eye(n, device=dev))).requires_grad_(True)
        state = {}

        def finish(ll, reward):
            loss = deepaco_loss({"reward": reward.view(ants, batch).t(), "log_likelihood": ll.view(ants, batch).t()})
            heat.grad = None
            loss.backward()
            state["grad"], state["length"] = heat.grad, -reward.double().mean()
            return state["grad"]

        def kernels():
            out = heatmap_rollout(heat, locs, n_ants=ants, seed=1234)
            return finish(out["log_likelihood"], out["reward"])

        def per_step():
            return finish(*torch_train_step(heat, locs, ants))

        legs = [Leg("kernels", kernels), Leg("torch_per_step", per_step)]
        for it in range(a.reps + 1):  # one warm-up round; the legs alternate inside every round
            for leg in legs:
                leg.launch(keep=it >= 1)
        results = []
        for leg in legs:
            t = sorted(leg.times)
            if not bool(torch.isfinite(leg.tours).all()) or float(leg.tours.abs().max()) == 0.0:
                raise SystemExit(f"aco_bench --train: leg {leg.kind} produced no usable gradient; no time is recorded")
            results.append(dict(leg=leg.kind, case=f"tsp{n}x{batch}", batch=batch, relation_to_cus=f"{batch} instances, {cus} CUs",
                                reps=len(t), median_ms=t[len(t) // 2], min_ms=t[0], max_ms=t[-1]))
        ratio = results[1]["median_ms"] / results[0]["median_ms"]
        for r in results:
            r["torch_over_kernels_median"] = ratio
            rows_out.append(r)
            print(json.dumps(r), flush=True)
    out = a.out or "profiles/aco_train_bench.json"
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), when=time.strftime("%Y-%m-%d"),
                       case=f"tsp{n}, {ants} ants, batches {list(batches)}, free heatmap -log(distance)",
                       what="training decode forward + deepaco_loss + backward to the heatmap (host work included), HIP events "
                            "around the step, synchronised; torch_per_step is this script's torch loop with autograd on the same "
                            "card (it draws other tours than the kernel); no threshold was fixed in advance",
                       rows=rows_out), f, indent=1)


def depot_instances(env, batch, n, dev):
    """Seeded instances in the generators' spirit (uniform locs; CVRP demands U{1..9} / 50; OP prizes by distance to the depot
    and the per-node table of budget 4; PCTSP prizes U(0, 4 / C), penalties U(0, 3 / C))."""
    g = torch.Generator().manual_seed(1234)
    c = n - 1
    locs = torch.rand(batch, n, 2, generator=g)
    to_depot = (locs[:, 0:1] - locs).norm(p=2, dim=-1)
    if env == "cvrp":
        td = {"demand": torch.randint(1, 10, (batch, c), generator=g).float() / 50, "vehicle_capacity": torch.ones(batch, 1)}
    elif env == "op":
        prize = (1 + (to_depot / to_depot.max(-1, keepdim=True).values * 99).int()).float() / 100
        prize[:, 0] = 0
        td = {"prize": prize, "max_length": torch.full((batch, 1), 4.0) - to_depot - 1e-6}
    else:
        prize, penalty = torch.rand(batch, n, generator=g) * (4.0 / c), torch.rand(batch, n, generator=g) * (3.0 / c)
        prize[:, 0] = 0
        penalty[:, 0] = 0
        td = {"real_prize": prize, "penalty": penalty}
    td["locs"] = locs
    return {k: v.to(dev) for k, v in td.items()}


def torch_depot_train_step(env, heat, td, n_ants, temperature=1.0):
    """The reference's training decode on a depot graph from torch ops with autograd, one decoding step at a time until every
    row is done (ant-major rows, every ant starts at the depot): the environment's mask, gather the row, log-softmax,
    multinomial, gather the log-prob. Returns (log_likelihood [rows], actions [rows, T])."""
    b, n, _ = heat.shape
    rows, dev = n_ants * b, heat.device
    ar, inst = torch.arange(rows, device=dev), torch.arange(rows, device=dev) % b
    locs = td["locs"][inst]
    cur = torch.zeros(rows, dtype=torch.int64, device=dev)
    visited = torch.zeros(rows, n, dtype=torch.bool, device=dev)
    acc = torch.zeros(rows, device=dev)
    done = torch.zeros(rows, dtype=torch.bool, device=dev)
    if env == "cvrp":
        demand = torch.cat((torch.zeros(b, 1, device=dev), td["demand"]), 1)[inst]
        cap = td["vehicle_capacity"].reshape(-1)[inst]
    steps, logps, t = [], [], 0
    while not bool(done.all()):
        if env == "cvrp":
            bad = visited | (demand + acc[:, None] > cap[:, None] + 1e-5)
            bad[:, 0] = (cur == 0) & ~bad[:, 1:].all(1)
        elif env == "op":
            reach = acc[:, None] + (locs - locs[ar, cur][:, None]).norm(p=2, dim=-1)
            bad = visited | visited[:, 0:1] | (reach > td["max_length"][inst])
            bad[:, 0] = False
        else:
            bad = visited | visited[:, 0:1]
            bad[:, 0] = (acc < 1.0) & ~visited[:, 1:].all(1)
        bad = torch.where(done[:, None], torch.arange(n, device=dev)[None, :] != 0, bad)  # a finished row stays at the depot
        lp = torch.log_softmax(heat[inst, cur].masked_fill(bad, float("-inf")) / temperature, -1)
        nxt = torch.multinomial(lp.detach().exp(), 1).squeeze(1)
        logps.append(lp[ar, nxt])
        if env == "cvrp":
            acc = (acc + demand[ar, nxt]) * (nxt != 0)
            visited = visited.clone()
            visited[ar, nxt] = True
            done = visited[:, 1:].all(1) & visited[:, 0]
        else:
            acc = acc + ((locs[ar, nxt] - locs[ar, cur]).norm(p=2, dim=-1) if env == "op" else td["real_prize"][inst, nxt])
            visited = visited.clone()
            visited[ar, nxt] = True
            done = done | ((nxt == 0) & (t > 0))
        cur = nxt
        steps.append(nxt)
        t += 1
    return torch.stack(logps, 1).sum(1), torch.stack(steps, 1)


def main_train_depot(a, dev):
    """``--train --env cvrp|op|pctsp``: ``main_train``'s protocol on a depot graph. Both legs take their reward from the same
    expression on their own rows (the tour length of [depot, row] closed; OP and PCTSP add their prize / penalty terms)."""
    from rl4co_amd.aco import deepaco_loss, heatmap_rollout

    env, n = a.env, a.num_loc + 1
    ants = 30 if a.ants is None else a.ants
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    batches = (64, 512) if a.batch is None else (a.batch,)
    rows_out = []
    for batch in batches:
        td = depot_instances(env, batch, n, dev)
        locs = td["locs"]
        dist = (locs[:, :, None] - locs[:, None, :]).norm(p=2, dim=-1)
        heat = (-torch.log(dist + 1e9 * torch.eye(n, device=dev))).requires_grad_(True)
        inst = torch.arange(ants * batch, device=dev) % batch
        state = {}

        def reward_of(actions):
            idx = torch.cat((torch.zeros_like(actions[:, :1]), actions), 1)
            pts = locs[inst[:, None], idx]
            length = (pts.roll(-1, 1) - pts).norm(p=2, dim=-1).sum(1)
            if env == "cvrp":
                return -length
            if env == "op":
                return td["prize"][inst[:, None], actions].sum(1)
            penalty = td["penalty"]
            return penalty[inst[:, None], actions].sum(1) - (length + penalty[:, 1:].sum(1)[inst])

        def finish(ll, reward):
            loss = deepaco_loss({"reward": reward.view(ants, batch).t(), "log_likelihood": ll.view(ants, batch).t()})
            heat.grad = None
            loss.backward()
            state["grad"] = heat.grad
            return state["grad"]

        def kernels():
            out = heatmap_rollout(heat, locs, n_ants=ants, seed=1234, env_name=env, td=td)
            state["kernel_steps"] = out["actions"].shape[1]
            return finish(out["log_likelihood"], out["reward"])

        def per_step():
            ll, actions = torch_depot_train_step(env, heat, td, ants)
            state["torch_steps"] = actions.shape[1]
            return finish(ll, reward_of(actions))

        legs = [Leg("kernels", kernels), Leg("torch_per_step", per_step)]
        for it in range(a.reps + 1):  # one warm-up round; the legs alternate inside every round
            for leg in legs:
                leg.launch(keep=it >= 1)
        results = []
        for leg in legs:
            t = sorted(leg.times)
            if not bool(torch.isfinite(leg.tours).all()) or float(leg.tours.abs().max()) == 0.0:
                raise SystemExit(f"aco_bench --train: leg {leg.kind} produced no usable gradient; no time is recorded")
            results.append(dict(leg=leg.kind, env=env, case=f"{env}{n - 1}x{batch}", batch=batch,
                                relation_to_cus=f"{batch} instances, {cus} CUs", reps=len(t), median_ms=t[len(t) // 2],
                                min_ms=t[0], max_ms=t[-1], row_width=state["kernel_steps"], torch_steps=state["torch_steps"]))
        ratio = results[1]["median_ms"] / results[0]["median_ms"]
        for r in results:
            r["torch_over_kernels_median"] = ratio
            rows_out.append(r)
            print(json.dumps(r), flush=True)
    out = a.out or "profiles/aco_depot_train_bench.json"
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    kept = []
    if os.path.exists(out):  # the other environments' rows stay
        with open(out) as f:
            kept = [r for r in json.load(f).get("rows", []) if r.get("env") != env]
    with open(out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), when=time.strftime("%Y-%m-%d"),
                       case=f"{n - 1} customers, {ants} ants, batches {list(batches)}, free heatmap -log(distance), every ant "
                            f"starts at the depot",
                       what="training decode forward + deepaco_loss + backward to the heatmap (host work included), HIP events "
                            "around the step, synchronised; torch_per_step is this script's torch loop with autograd on the same "
                            "card (it draws other rows than the kernel, torch_steps of them against the kernel's fixed "
                            "row_width); no threshold was fixed in advance",
                       rows=kept + rows_out), f, indent=1)


if __name__ == "__main__":
    main()
