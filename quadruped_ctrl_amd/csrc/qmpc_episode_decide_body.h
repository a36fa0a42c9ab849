// qmpc_episode_decide_body.h -- the statements of one lane of the episode manager's decision, as TEXT: included inside the
// body of a decision kernel (qmpc_episode.hip: every robot is judged; qmpc_episode_sense.hip: a robot in warm-up is not),
// for the reason qmpc_plant_step_body.h gives, with in scope
//   #pragma clang fp contract(off) at the head of the kernel's body (the pragma is only allowed there);
//   qmpc_episode.h and qmpc_episode_rule.h;
//   the kernel's parameters S (QmpcEpisodeDev), In (QmpcEpisodeIn), R (qmpc_episode_rule), Bd (qmpc_episode_bind), elapsed;
//   const int b, the lane's robot, and const bool judge: the robot exists and is judged by this step.
// No include guard: it is included once per kernel.  It has no return: EVERY lane of every wave reaches the ballot, judged
// or not, and the kernel's own statements may follow it.  Behind it `done` says whether the lane's robot finished an
// episode here.  A lane with judge == false reads and writes nothing (its mask[b] is the including kernel's business).
  int cause = 0, age = 0;
  QmpcEpisodeFacts F{};
  if (judge) {
    double p[3], q[4], start[2];
    for (int k = 0; k < 3; ++k) p[k] = In.p[(size_t)b * 3 + k];
    for (int k = 0; k < 4; ++k) q[k] = In.q[(size_t)b * 4 + k];
    for (int k = 0; k < 2; ++k) start[k] = S.start[(size_t)b * 2 + k];
    const double ground = In.ground ? In.ground[b] : 0.0;
    age = qmpc_episode_age(S.age[b], elapsed);
    cause = qmpc_episode_cause(R, In.safe[b], p, q, ground, start, age, &F);
  }
  const bool done = cause != 0;
  const int episode = done ? S.episode[b] : 0;
  if (Bd.log) {
    // the wave's done lanes take consecutive rows; a row at or beyond log_rows is not written
    const unsigned long long m = __ballot(done);
    if (m) {
      const int lane = (int)__lane_id(), leader = __ffsll(m) - 1, n = __popcll(m);
      int base = 0;
      if (lane == leader) {
        base = atomicAdd(S.log_words, n);
        const long long end = (long long)base + n, cap = (long long)Bd.log_rows;
        if (end > cap) {
          const int beyond = (int)(end - (base > cap ? (long long)base : cap));
          atomicSub(S.log_words, beyond);
          atomicAdd(S.log_words + 1, beyond);
        }
      }
      base = __shfl(base, leader);
      const long long row = (long long)base + __popcll(m & ((1ull << lane) - 1ull));
      if (done && row < (long long)Bd.log_rows) {
        double* out = Bd.log + (size_t)row * 8;
        out[0] = (double)b;
        out[1] = (double)episode;
        out[2] = (double)cause;
        out[3] = (double)age;
        out[4] = F.dx;
        out[5] = F.dy;
        out[6] = F.height;
        out[7] = F.tilt;
      }
    }
  }
  if (judge && !done) {
    S.age[b] = age;
    S.mask[b] = 0;
  }
  if (done) {
    for (int k = 0; k < QMPC_EP_CAUSES; ++k)
      if (cause & (1 << k)) S.count[(size_t)b * QMPC_EP_CAUSES + k] += 1;
    S.ticks_sum[b] += (int64_t)age;
    S.last_cause[b] = cause;
    S.last_ticks[b] = age;
    const int next = (int)((uint32_t)episode + 1u);
    int spawn_row, command_row;
    qmpc_episode_draw(In.key0, In.key1, b, next, Bd.n_spawn, Bd.commands ? Bd.n_commands : 0, &spawn_row, &command_row);
    const double* sp = Bd.spawn + qmpc_episode_spawn_at(b, spawn_row, Bd.n_spawn, Bd.flags);
    const double x = sp[0], y = sp[1];
    S.xyyaw[(size_t)b * 3 + 0] = x;
    S.xyyaw[(size_t)b * 3 + 1] = y;
    S.xyyaw[(size_t)b * 3 + 2] = sp[2];
    S.start[(size_t)b * 2 + 0] = x;
    S.start[(size_t)b * 2 + 1] = y;
    S.mask[b] = 1;
    S.age[b] = 0;
    S.episode[b] = next;
    if (Bd.commands) {
      const double* cm = Bd.commands + (size_t)command_row * 4;
      for (int k = 0; k < 3; ++k) Bd.vel[(size_t)b * 3 + k] = cm[k];
      Bd.gait[b] = qmpc_episode_gait(cm[3]);
    }
  }
