"""The CTC loss of one utterance and its gradient with respect to the logits, restated in fp64 numpy with plain loops (tests
only).  Notation of parrot_tts_amd/csrc/ctc.h: the S = 2 N + 1 states blank, tok_0, blank, ..., blank; lp = log_softmax(logits);

    alpha_0[0] = lp[0][blank], alpha_0[1] = lp[0][tok_0]
    alpha_t[s] = logaddexp(alpha_{t-1}[s], alpha_{t-1}[s-1], alpha_{t-1}[s-2] if skip_s) + lp[t][label_s]
    nll        = -logaddexp(alpha_{T-1}[S-1], alpha_{T-1}[S-2])
    beta_{T-1}[S-1] = lp[T-1][blank], beta_{T-1}[S-2] = lp[T-1][label_{S-2}]
    beta_t[s]  = logaddexp(beta_{t+1}[s], beta_{t+1}[s+1], beta_{t+1}[s+2] if skip_{s+2}) + lp[t][label_s]
    gamma_t(v) = sum_{s : label_s = v} exp(alpha_t[s] + beta_t[s] - lp[t][v] + nll)
    grad[t][v] = w (exp(lp[t][v]) - gamma_t(v))

skip_s: s is odd and its token differs from the token before it.  This is the true gradient: it agrees with central differences
of its own nll also where the last token is the blank, where torch's CPU backward does not."""
import numpy as np

NINF = -np.inf


def _logaddexp(*xs):
    m = max(xs)
    if m == NINF:
        return NINF
    return m + np.log(sum(np.exp(x - m) for x in xs))


def log_softmax(logits, lse=None):
    """lp (T, V) fp64; ``lse`` (T): a given log-sum-exp per frame (the device's fp32 one) instead of the fp64 one."""
    x = np.asarray(logits, dtype=np.float64)
    if lse is None:
        m = x.max(axis=1, keepdims=True)
        lse = (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]
    return x - np.asarray(lse, dtype=np.float64)[:, None]


def _states(tokens):
    N = len(tokens)
    S = 2 * N + 1
    label = [0] * S
    skip = [False] * S
    for j in range(N):
        label[2 * j + 1] = int(tokens[j])
        skip[2 * j + 1] = j > 0 and int(tokens[j]) != int(tokens[j - 1])
    return S, label, skip


def ctc_nll(logits, tokens, lse=None):
    """-log p(tokens | logits) of one utterance: logits (T, V), tokens (N); +inf when there is no path."""
    lp = log_softmax(logits, lse)
    T = lp.shape[0]
    S, label, skip = _states(tokens)
    a = [NINF] * S
    a[0], a[1] = lp[0][0], lp[0][label[1]]
    for t in range(1, T):
        p = a
        a = [NINF] * S
        for s in range(S):
            terms = [p[s]]
            if s >= 1:
                terms.append(p[s - 1])
            if s >= 2 and skip[s]:
                terms.append(p[s - 2])
            a[s] = _logaddexp(*terms) + lp[t][label[s]]
    return -_logaddexp(a[S - 1], a[S - 2])


def ctc_nll_and_grad(logits, tokens, w=1.0, lse=None):
    """(nll, grad (T, V) fp64) of one utterance, grad = w d nll / d logits.  A row without a path: (+inf, all NaN)."""
    lp = log_softmax(logits, lse)
    T, V = lp.shape
    S, label, skip = _states(tokens)
    alpha = np.full((T, S), NINF)
    beta = np.full((T, S), NINF)
    alpha[0][0], alpha[0][1] = lp[0][0], lp[0][label[1]]
    for t in range(1, T):
        for s in range(S):
            terms = [alpha[t - 1][s]]
            if s >= 1:
                terms.append(alpha[t - 1][s - 1])
            if s >= 2 and skip[s]:
                terms.append(alpha[t - 1][s - 2])
            alpha[t][s] = _logaddexp(*terms) + lp[t][label[s]]
    nll = -_logaddexp(alpha[T - 1][S - 1], alpha[T - 1][S - 2])
    if nll == np.inf:
        return nll, np.full((T, V), np.nan)
    beta[T - 1][S - 1], beta[T - 1][S - 2] = lp[T - 1][0], lp[T - 1][label[S - 2]]
    for t in range(T - 2, -1, -1):
        for s in range(S):
            terms = [beta[t + 1][s]]
            if s + 1 < S:
                terms.append(beta[t + 1][s + 1])
            if s + 2 < S and skip[s + 2]:
                terms.append(beta[t + 1][s + 2])
            beta[t][s] = _logaddexp(*terms) + lp[t][label[s]]
    grad = np.zeros((T, V))
    for t in range(T):
        gamma = [0.0] * V
        for s in range(S):
            gamma[label[s]] += np.exp(alpha[t][s] + beta[t][s] - lp[t][label[s]] + nll)
        for v in range(V):
            grad[t][v] = w * (np.exp(lp[t][v]) - gamma[v])
    return nll, grad
